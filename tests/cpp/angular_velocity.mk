# Driver of the facade's angular-velocity side (tracker::AngularVelocityEstimator of feature_tracker/angular_velocity.h).
# Run from this directory:  make -f angular_velocity.mk [OUT=<dir>] <target>   (OUT: where the binary goes; default here).
# Host compiler only.  Used by tests/test_gpu_rotation_facade.py.
CXX ?= g++
ROOT = ../..
OUT ?= .
LIBDIR = $(abspath $(ROOT)/event-based-odomety_amd)
FACADE = $(ROOT)/include/ebo.h $(wildcard $(ROOT)/event-based-odomety_amd/include/*/*.h)
LINK = -L$(LIBDIR) -lebo_hip -Wl,-rpath,$(LIBDIR) -Wl,-rpath,/opt/rocm/lib
FLAGS = -std=c++17 -O2 -ffp-contract=off -Wall -Wextra -I$(ROOT)/event-based-odomety_amd/include

.PHONY: all
all: $(OUT)/angular_velocity_test

$(OUT)/angular_velocity_test: angular_velocity_test.cpp $(FACADE)
	$(CXX) $(FLAGS) -o $@ angular_velocity_test.cpp $(LINK)
