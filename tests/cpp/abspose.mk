# Driver of the odometry front end (visual_odometry/visual_odometry.h over two_view.h, keyframe.h, common::Pose3d).
# Run from this directory:  make -f abspose.mk [OUT=<dir>] <target>   (OUT: where the binary goes; default here).
# Host compiler only; -ffp-contract=off: one rounding per operation, as the library and tests/abspose_ref.py.
# Used by tests/test_abspose_cpu.py (the host-only `self` mode) and tests/test_gpu_odometry_facade.py.
CXX ?= g++
ROOT = ../..
OUT ?= .
LIBDIR = $(abspath $(ROOT)/event-based-odomety_amd)
FACADE = $(ROOT)/include/ebo.h $(wildcard $(ROOT)/event-based-odomety_amd/include/*/*.h)
LINK = -L$(LIBDIR) -lebo_hip -Wl,-rpath,$(LIBDIR) -Wl,-rpath,/opt/rocm/lib
FLAGS = -std=c++17 -O2 -ffp-contract=off -Wall -Wextra -I$(ROOT)/event-based-odomety_amd/include

.PHONY: all
all: $(OUT)/localize_lines_test

$(OUT)/localize_lines_test: localize_lines_test.cpp $(FACADE)
	$(CXX) $(FLAGS) -o $@ localize_lines_test.cpp $(LINK)
