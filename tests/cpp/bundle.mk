# Driver of the façade's bundle-adjustment members (visual_odometry/bundle_adjustment.h, VisualOdometryFrontEnd).
# Run from this directory:  make -f bundle.mk [OUT=<dir>] <target>   (OUT: where the binary goes; default here).
# Host compiler only; -ffp-contract=off: one rounding per operation, as the library and tests/bundle_ref.py.
# Used by tests/test_gpu_bundle_facade.py and tests/test_gpu_bundle_frontend.py.
CXX ?= g++
ROOT = ../..
OUT ?= .
LIBDIR = $(abspath $(ROOT)/event-based-odomety_amd)
FACADE = $(ROOT)/include/ebo.h $(wildcard $(ROOT)/event-based-odomety_amd/include/*/*.h)
LINK = -L$(LIBDIR) -lebo_hip -Wl,-rpath,$(LIBDIR) -Wl,-rpath,/opt/rocm/lib
FLAGS = -std=c++17 -O2 -ffp-contract=off -Wall -Wextra -I$(ROOT)/event-based-odomety_amd/include

.PHONY: all
all: $(OUT)/bundle_lines_test

$(OUT)/bundle_lines_test: bundle_lines_test.cpp $(FACADE)
	$(CXX) $(FLAGS) -o $@ bundle_lines_test.cpp $(LINK)
