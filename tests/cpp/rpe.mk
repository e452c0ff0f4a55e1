# Driver of the facade's relative-pose-error side (relativePoseErrors, relativePoseErrorsPrefixes of visual_odometry/aligner.h,
# useDeviceRelativeErrors of VisualOdometryFrontEnd).
# Run from this directory:  make -f rpe.mk [OUT=<dir>] <target>   (OUT: where the binary goes; default here).
# Host compiler only; -ffp-contract=off: one rounding per operation, as the library and tests/rpe_ref.py.
# Used by tests/test_gpu_rpe_facade.py.
CXX ?= g++
ROOT = ../..
OUT ?= .
LIBDIR = $(abspath $(ROOT)/event-based-odomety_amd)
FACADE = $(ROOT)/include/ebo.h $(wildcard $(ROOT)/event-based-odomety_amd/include/*/*.h)
LINK = -L$(LIBDIR) -lebo_hip -Wl,-rpath,$(LIBDIR) -Wl,-rpath,/opt/rocm/lib
FLAGS = -std=c++17 -O2 -ffp-contract=off -Wall -Wextra -I$(ROOT)/event-based-odomety_amd/include

.PHONY: all
all: $(OUT)/rpe_facade_test

$(OUT)/rpe_facade_test: rpe_facade_test.cpp $(FACADE)
	$(CXX) $(FLAGS) -o $@ rpe_facade_test.cpp $(LINK)
