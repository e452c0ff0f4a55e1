# Driver of the facade's map-maintenance side (maintainMap of visual_odometry/map_maintenance.h, useDeviceMapMaintenance
# of VisualOdometryFrontEnd).
# Run from this directory:  make -f map_maintenance.mk [OUT=<dir>] <target>   (OUT: where the binary goes; default here).
# Host compiler only; -ffp-contract=off: one rounding per operation, as the library and tests/landmark_ref.py.
# Used by tests/test_gpu_map_maintenance_facade.py.
CXX ?= g++
ROOT = ../..
OUT ?= .
LIBDIR = $(abspath $(ROOT)/event-based-odomety_amd)
FACADE = $(ROOT)/include/ebo.h $(wildcard $(ROOT)/event-based-odomety_amd/include/*/*.h)
LINK = -L$(LIBDIR) -lebo_hip -Wl,-rpath,$(LIBDIR) -Wl,-rpath,/opt/rocm/lib
FLAGS = -std=c++17 -O2 -ffp-contract=off -Wall -Wextra -I$(ROOT)/event-based-odomety_amd/include

.PHONY: all
all: $(OUT)/map_maintenance_test

$(OUT)/map_maintenance_test: map_maintenance_test.cpp $(FACADE)
	$(CXX) $(FLAGS) -o $@ map_maintenance_test.cpp $(LINK)
