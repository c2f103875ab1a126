# jpge build (no cmake needed).  `make -j8` builds:
#   jpgenc_amd/lib/libjpge.so   the product: HIP kernels for gfx950 + host C++ + C ABI
#   jpgenc_amd/bin/jpgenc       the CLI (reference main.cpp contract)
#   oracle/build/liborc.so      test-only CPU restatement (+ oracle/_ref when /root/reference exists)
ROCM     ?= /opt/rocm
HIPCC    ?= $(ROCM)/bin/hipcc
CXX      ?= g++
ARCH     ?= gfx950
BUILD    ?= build/obj
SRC      := jpgenc_amd/csrc
LIBDIR   ?= jpgenc_amd/lib
BINDIR   := jpgenc_amd/bin

HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -I$(SRC) -Iinclude $(HIPEXTRA)
CXXFLAGS := -O2 -std=c++17 -fPIC -pthread -Wall -Wextra -Wno-unused-parameter -Wno-unused-result \
            -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -I$(SRC) -Iinclude $(HIPEXTRA)

HOST_SRCS := encoder.cpp frame_plan.cpp encoder_stripes.cpp encoder_planes.cpp capi.cpp host_io.cpp huffman.cpp jpge_image.cpp ingest.cpp host_decode.cpp coding.cpp group.cpp
HOST_OBJS := $(addprefix $(BUILD)/,$(HOST_SRCS:.cpp=.o))
# (fdct_*_d2 / _d4: the shapes' box-downscaling builds, jpge_set_downscale)
K1_DS_SRCS := fdct_rgb8_d2.hip fdct_rgb8_d4.hip fdct_bgr8_d2.hip fdct_bgr8_d4.hip fdct_x4_d2.hip fdct_x4_d4.hip fdct_nv12_d2.hip fdct_nv12_d4.hip
# (fdct_*_o1 .. _o4: the shapes' oriented builds, jpge_set_orientation)
K1_OR_SRCS := $(foreach s,rgb8 bgr8 x4,$(foreach c,1 2 3 4,fdct_$(s)_o$(c).hip))
# (fdct_*_lut: the shapes' builds that map each staged pixel through the context's channel tables, jpge_set_channel_lut)
K1_LUT_SRCS := fdct_rgb8_lut.hip fdct_bgr8_lut.hip fdct_x4_lut.hip fdct_bayer8_lut.hip
DEV_SRCS  := fdct.hip fdct_bgr8.hip fdct_x4.hip fdct_planar.hip fdct_nv12.hip fdct_i420.hip fdct_yuv444.hip fdct_gray.hip fdct_packed422.hip fdct_nv16.hip fdct_i422.hip fdct_p010.hip fdct_i010.hip fdct_y210.hip fdct_p210.hip fdct_i210.hip fdct_v210.hip fdct_bayer8.hip $(K1_DS_SRCS) $(K1_OR_SRCS) $(K1_LUT_SRCS) stats.hip entropy.hip planes.hip concat.hip
DEV_OBJS  := $(addprefix $(BUILD)/,$(DEV_SRCS:.hip=.o))
DIAG_OBJS := $(addprefix $(BUILD)/diag/,$(DEV_SRCS:.hip=.o))
HEADERS   := $(wildcard $(SRC)/*.hpp) include/jpge.h
FACADE_TEST := tests/cpp/bin/test_facade
HUFF_TEST   := tests/cpp/bin/test_huffman_fast
QUANT_TEST  := tests/cpp/bin/test_quant_fast
EXIT_TEST   := tests/cpp/bin/test_exit_close
HUFFSPEC_TEST := tests/cpp/bin/test_huffspec
YUVXF_TEST  := tests/cpp/bin/test_yuvxf
PLAN_TEST   := tests/cpp/bin/test_frame_plan
PLAN_DEPS   := tests/cpp/test_frame_plan.cpp $(SRC)/frame_plan.cpp $(SRC)/frame_plan.hpp $(SRC)/layouts.hpp $(SRC)/kernels.hpp $(SRC)/host_io.hpp

all: $(LIBDIR)/libjpge.so $(BINDIR)/jpgenc $(FACADE_TEST) $(HUFF_TEST) $(QUANT_TEST) $(EXIT_TEST) $(HUFFSPEC_TEST) $(YUVXF_TEST) $(PLAN_TEST) oracle

# (fdct_*.hip: fdct.hip built per input load shape)
K1_SHAPES := fdct_bgr8.o fdct_x4.o fdct_planar.o fdct_nv12.o fdct_i420.o fdct_yuv444.o fdct_gray.o fdct_packed422.o fdct_nv16.o fdct_i422.o fdct_p010.o fdct_i010.o fdct_y210.o fdct_p210.o fdct_i210.o fdct_v210.o fdct_bayer8.o $(K1_DS_SRCS:.hip=.o) $(K1_OR_SRCS:.hip=.o) $(K1_LUT_SRCS:.hip=.o)
$(addprefix $(BUILD)/,$(K1_SHAPES)) $(addprefix $(BUILD)/diag/,$(K1_SHAPES)): $(SRC)/fdct.hip

$(BUILD)/%.o: $(SRC)/%.hip $(HEADERS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/diag/%.o: $(SRC)/%.hip $(HEADERS)
	@mkdir -p $(BUILD)/diag
	$(HIPCC) $(HIPFLAGS) -DJPGE_STAMPS -c $< -o $@

$(BUILD)/%.o: $(SRC)/%.cpp $(HEADERS)
	@mkdir -p $(BUILD)
	$(CXX) $(CXXFLAGS) -c $< -o $@

$(LIBDIR)/libjpge.so: $(DEV_OBJS) $(HOST_OBJS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -pthread -o $@ $^ -L$(ROCM)/lib -lamdhip64 -ldl

$(BINDIR)/jpgenc: $(SRC)/cli.cpp $(LIBDIR)/libjpge.so
	@mkdir -p $(BINDIR)
	$(CXX) $(CXXFLAGS) -o $@ $< -L$(LIBDIR) -ljpge -Wl,-rpath,'$$ORIGIN/../lib' \
	  -L$(ROCM)/lib -lamdhip64 -Wl,-rpath,$(ROCM)/lib

oracle:
	$(MAKE) -C oracle

# diagnostic build with in-kernel phase stamps (JPGE_LIB=jpgenc_amd/lib/diag/libjpge.so,
# JPGE_STAMPS_FILE=<path>); never used by tests or the bench
diag: $(DIAG_OBJS) $(HOST_OBJS)
	@mkdir -p $(LIBDIR)/diag
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -pthread -o $(LIBDIR)/diag/libjpge.so $^ \
	  -L$(ROCM)/lib -lamdhip64

clean:
	rm -rf build $(LIBDIR) $(BINDIR) tests/cpp/bin
	$(MAKE) -C oracle clean

.PHONY: all oracle clean

# the facade under the reference's unit tests (tests/cpp/test_facade.cpp; run by
# tests/test_facade.py): compiled exactly as reference code would be, global names
$(FACADE_TEST): tests/cpp/test_facade.cpp $(LIBDIR)/libjpge.so $(SRC)/jpge_image.hpp include/jpge.h
	@mkdir -p tests/cpp/bin
	$(CXX) $(CXXFLAGS) -o $@ $< -L$(LIBDIR) -ljpge -Wl,-rpath,'$$ORIGIN/../../../$(LIBDIR)' \
	  -L$(ROCM)/lib -lamdhip64 -Wl,-rpath,$(ROCM)/lib

# a caller's exit-time close after the library's own exit handler (tests/test_gpu_teardown.py)
$(EXIT_TEST): tests/cpp/test_exit_close.cpp $(LIBDIR)/libjpge.so include/jpge.h
	@mkdir -p tests/cpp/bin
	$(CXX) $(CXXFLAGS) -o $@ $< -L$(LIBDIR) -ljpge -Wl,-rpath,'$$ORIGIN/../../../$(LIBDIR)' \
	  -L$(ROCM)/lib -lamdhip64 -Wl,-rpath,$(ROCM)/lib

# the Huffman table builder's array emulation against the standard containers
# (tests/test_host.py runs it)
$(HUFF_TEST): tests/cpp/test_huffman_fast.cpp $(SRC)/huffman.cpp $(SRC)/huffman.hpp
	@mkdir -p tests/cpp/bin
	$(CXX) $(CXXFLAGS) -o $@ $< $(SRC)/huffman.cpp

# K1's quantiser fast path against the reference's two roundings (tests/test_host.py runs it)
$(QUANT_TEST): tests/cpp/test_quant_fast.cpp $(SRC)/constants.hpp
	@mkdir -p tests/cpp/bin
	$(CXX) -O2 -std=c++17 -ffp-contract=off -I$(SRC) -o $@ $<

# fixed Huffman tables: spec validation and canonical codes, host only
# (tests/test_fixedhuff_cpu.py runs it)
$(HUFFSPEC_TEST): tests/cpp/test_huffspec.cpp $(SRC)/host_io.cpp $(SRC)/host_io.hpp $(SRC)/huffman.hpp $(SRC)/host_par.hpp
	@mkdir -p tests/cpp/bin
	$(CXX) $(CXXFLAGS) -o $@ $< $(SRC)/host_io.cpp

# the sample transform of Y, Cb, Cr input: the setting's validation and the presets, host only
# (tests/test_yuvxf_cpu.py runs it)
$(YUVXF_TEST): tests/cpp/test_yuvxf.cpp $(SRC)/host_io.cpp $(SRC)/host_io.hpp $(SRC)/huffman.hpp $(SRC)/host_par.hpp
	@mkdir -p tests/cpp/bin
	$(CXX) $(CXXFLAGS) -o $@ $< $(SRC)/host_io.cpp

# the layout table, the frame plan's refusals and its upload layout, host only: no HIP library
# is linked (tests/test_frame_plan_cpu.py runs it)
$(PLAN_TEST): $(PLAN_DEPS)
	@mkdir -p tests/cpp/bin
	$(CXX) $(CXXFLAGS) -o $@ $< $(SRC)/frame_plan.cpp

# Host code under AddressSanitizer + UndefinedBehaviorSanitizer (run by
# tests/test_asan.py in the CPU suite): every host .cpp of the library rebuilt
# sanitized and linked with the (unsanitized) HIP device objects, plus the host
# tests.  No GPU is touched: the drivers call host-only entry points.
ASAN_FLAGS := -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1
ASAN_DIR   := build/asan
ASAN_BIN   := tests/cpp/bin/asan
ASAN_OBJS  := $(addprefix $(ASAN_DIR)/,$(HOST_SRCS:.cpp=.o))
ASAN_TESTS := $(ASAN_BIN)/test_host_asan $(ASAN_BIN)/test_facade $(ASAN_BIN)/test_huffman_fast $(ASAN_BIN)/test_quant_fast \
              $(ASAN_BIN)/test_huffspec $(ASAN_BIN)/test_yuvxf $(ASAN_BIN)/test_frame_plan

$(ASAN_DIR)/%.o: $(SRC)/%.cpp $(HEADERS)
	@mkdir -p $(ASAN_DIR)
	$(CXX) $(CXXFLAGS) $(ASAN_FLAGS) -c $< -o $@

$(ASAN_BIN)/test_host_asan: tests/cpp/test_host_asan.cpp $(ASAN_OBJS) $(DEV_OBJS)
	@mkdir -p $(ASAN_BIN)
	$(CXX) $(CXXFLAGS) $(ASAN_FLAGS) -o $@ $^ -L$(ROCM)/lib -lamdhip64 -ldl -Wl,-rpath,$(ROCM)/lib

$(ASAN_BIN)/test_facade: tests/cpp/test_facade.cpp $(ASAN_OBJS) $(DEV_OBJS)
	@mkdir -p $(ASAN_BIN)
	$(CXX) $(CXXFLAGS) $(ASAN_FLAGS) -o $@ $^ -L$(ROCM)/lib -lamdhip64 -ldl -Wl,-rpath,$(ROCM)/lib

$(ASAN_BIN)/test_huffman_fast: tests/cpp/test_huffman_fast.cpp $(SRC)/huffman.cpp $(SRC)/huffman.hpp
	@mkdir -p $(ASAN_BIN)
	$(CXX) $(CXXFLAGS) $(ASAN_FLAGS) -o $@ $< $(SRC)/huffman.cpp

$(ASAN_BIN)/test_quant_fast: tests/cpp/test_quant_fast.cpp $(SRC)/constants.hpp
	@mkdir -p $(ASAN_BIN)
	$(CXX) -std=c++17 -ffp-contract=off -I$(SRC) $(ASAN_FLAGS) -o $@ $<

$(ASAN_BIN)/test_huffspec: tests/cpp/test_huffspec.cpp $(SRC)/host_io.cpp $(SRC)/host_io.hpp $(SRC)/huffman.hpp $(SRC)/host_par.hpp
	@mkdir -p $(ASAN_BIN)
	$(CXX) $(CXXFLAGS) $(ASAN_FLAGS) -o $@ $< $(SRC)/host_io.cpp

$(ASAN_BIN)/test_yuvxf: tests/cpp/test_yuvxf.cpp $(SRC)/host_io.cpp $(SRC)/host_io.hpp $(SRC)/huffman.hpp $(SRC)/host_par.hpp
	@mkdir -p $(ASAN_BIN)
	$(CXX) $(CXXFLAGS) $(ASAN_FLAGS) -o $@ $< $(SRC)/host_io.cpp

$(ASAN_BIN)/test_frame_plan: $(PLAN_DEPS)
	@mkdir -p $(ASAN_BIN)
	$(CXX) $(CXXFLAGS) $(ASAN_FLAGS) -o $@ $< $(SRC)/frame_plan.cpp

asan: $(ASAN_TESTS)

.PHONY: asan
