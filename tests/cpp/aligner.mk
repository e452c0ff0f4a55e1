# Driver of the facade's ground-truth side (visual_odometry/aligner.h, the ground-truth members of VisualOdometryFrontEnd).
# Run from this directory:  make -f aligner.mk [OUT=<dir>] <target>   (OUT: where the binary goes; default here).
# Host compiler only; -ffp-contract=off: one rounding per operation, as the library and tests/align_ref.py.
# Used by tests/test_align_cpu.py (the host-only `self` and `sync` modes) and tests/test_gpu_align_facade.py.
CXX ?= g++
ROOT = ../..
OUT ?= .
LIBDIR = $(abspath $(ROOT)/event-based-odomety_amd)
FACADE = $(ROOT)/include/ebo.h $(wildcard $(ROOT)/event-based-odomety_amd/include/*/*.h)
LINK = -L$(LIBDIR) -lebo_hip -Wl,-rpath,$(LIBDIR) -Wl,-rpath,/opt/rocm/lib
FLAGS = -std=c++17 -O2 -ffp-contract=off -Wall -Wextra -I$(ROOT)/event-based-odomety_amd/include

.PHONY: all
all: $(OUT)/aligner_test

$(OUT)/aligner_test: aligner_test.cpp $(FACADE)
	$(CXX) $(FLAGS) -o $@ aligner_test.cpp $(LINK)
