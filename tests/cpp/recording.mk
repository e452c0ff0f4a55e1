# Drivers of the recording path (tools::Davis240cRecording, tools::Replayer, tools::Evaluator) and of the PNG decoder.
# Run from this directory:  make -f recording.mk [OUT=<dir>] <target>   (OUT: where the binaries go; default here).
# Host compiler only.  Used by tests/test_recording_cpu.py, tests/test_png8_cpu.py and tests/test_gpu_recording.py.
CXX ?= g++
ROOT = ../..
OUT ?= .
LIBDIR = $(abspath $(ROOT)/event-based-odomety_amd)
FACADE = $(ROOT)/include/ebo.h $(wildcard $(ROOT)/event-based-odomety_amd/include/*/*.h)
LINK = -L$(LIBDIR) -lebo_hip -Wl,-rpath,$(LIBDIR) -Wl,-rpath,/opt/rocm/lib

.PHONY: all
all: $(OUT)/recording_test $(OUT)/recording_opencv_test $(OUT)/png8_fuzz

# the recording driver against the facade (reference-style includes), linking the product library
$(OUT)/recording_test: recording_test.cpp $(FACADE)
	$(CXX) -std=c++17 -O1 -Wall -Wextra -I$(ROOT)/event-based-odomety_amd/include -o $@ recording_test.cpp $(LINK)

# the same program with the facade's EBO_HAVE_OPENCV branch live (test-only OpenCV declarations): Image8 is a cv::Mat
$(OUT)/recording_opencv_test: recording_test.cpp stubs_opencv/opencv2/core.hpp $(FACADE)
	$(CXX) -std=c++17 -O1 -Wall -Wextra -Istubs_opencv -I$(ROOT)/event-based-odomety_amd/include -o $@ recording_test.cpp $(LINK)

# csrc/png8.h alone (HIP-free) under AddressSanitizer + UBSan: truncations, byte flips and valid images
$(OUT)/png8_fuzz: png8_fuzz.cpp $(ROOT)/event-based-odomety_amd/csrc/png8.h $(ROOT)/include/ebo.h
	$(CXX) -std=c++17 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ png8_fuzz.cpp
