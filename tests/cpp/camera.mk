# Drivers of the camera model (common::CameraModel of the facade) and of the rectified replay.
# Run from this directory:  make -f camera.mk [OUT=<dir>] <target>   (OUT: where the binaries go; default here).
# Host compiler only; -ffp-contract=off: one rounding per operation, as the library and tests/camera_ref.py.
# Used by tests/test_camera_cpu.py and tests/test_gpu_camera.py.
CXX ?= g++
ROOT = ../..
OUT ?= .
LIBDIR = $(abspath $(ROOT)/event-based-odomety_amd)
FACADE = $(ROOT)/include/ebo.h $(wildcard $(ROOT)/event-based-odomety_amd/include/*/*.h)
LINK = -L$(LIBDIR) -lebo_hip -Wl,-rpath,$(LIBDIR) -Wl,-rpath,/opt/rocm/lib
FLAGS = -std=c++17 -O2 -ffp-contract=off -Wall -Wextra -I$(ROOT)/event-based-odomety_amd/include

.PHONY: all
all: $(OUT)/camera_model_lines_test $(OUT)/rectify_replay_test

$(OUT)/camera_model_lines_test: camera_model_lines_test.cpp $(FACADE)
	$(CXX) $(FLAGS) -o $@ camera_model_lines_test.cpp $(LINK)

# tools::EventPump with EvaluatorParams::rectifyEvents against the pump fed host-rectified events
$(OUT)/rectify_replay_test: rectify_replay_test.cpp $(FACADE)
	$(CXX) $(FLAGS) -o $@ rectify_replay_test.cpp $(LINK)
