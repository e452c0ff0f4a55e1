# Driver of the two-view facade's device refinement (visual_odometry/relative_refinement.h, two_view.h, visual_odometry.h).
# Run from this directory:  make -f twoview_refine.mk [OUT=<dir>] <target>   (OUT: where the binary goes; default here).
# Host compiler only; -ffp-contract=off: one rounding per operation, as the library and tests/twoview_ref.py.
# Used by tests/test_gpu_twoview_refine_facade.py.
CXX ?= g++
ROOT = ../..
OUT ?= .
LIBDIR = $(abspath $(ROOT)/event-based-odomety_amd)
FACADE = $(ROOT)/include/ebo.h $(wildcard $(ROOT)/event-based-odomety_amd/include/*/*.h)
LINK = -L$(LIBDIR) -lebo_hip -Wl,-rpath,$(LIBDIR) -Wl,-rpath,/opt/rocm/lib
FLAGS = -std=c++17 -O2 -ffp-contract=off -Wall -Wextra -I$(ROOT)/event-based-odomety_amd/include

.PHONY: all
all: $(OUT)/two_view_refine_test

$(OUT)/two_view_refine_test: two_view_refine_test.cpp $(FACADE)
	$(CXX) $(FLAGS) -o $@ two_view_refine_test.cpp $(LINK)
