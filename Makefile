# Builds libbirdnet_hip.so (gfx950 only) and the CPU oracle.
HIPCC ?= /opt/rocm/bin/hipcc
CXX := g++
ARCH ?= gfx950
PKG := rust-birdnet-onnx_amd
SRC := $(PKG)/csrc
OUT := $(PKG)/libbirdnet_hip.so
CXXFLAGS := -O3 -std=c++17 -fPIC -Wall -Wextra -Wno-unused-parameter -Iinclude
# -fno-slp-vectorize: left to itself the compiler packs neighbouring scalar f32 operations into v_pk_fma_f32 / v_pk_mul_f32 and pays
# for the pairs with register moves (mbmap's depthwise phase: 120 v_pk_fma + 216 v_mov for 240 multiply-adds); on this part a packed
# f32 instruction costs 1.56x a plain one (tools/mfma_valu_probe.cpp) and every vector instruction is paid out of the MFMA time
HIPFLAGS := $(CXXFLAGS) --offload-arch=$(ARCH) -ffp-contract=off -fno-slp-vectorize
OBJS := $(SRC)/onnx_proto.o $(SRC)/engine.o $(SRC)/onnx_rewrite.o $(SRC)/dft_bank.o $(SRC)/mbconv_fuse.o $(SRC)/plan_passes.o $(SRC)/detect.o $(SRC)/capi.o $(SRC)/recording.o $(SRC)/step_common.o $(SRC)/group.o $(SRC)/host_classifier.o $(SRC)/host_capi.o $(SRC)/host_rangefilter.o $(SRC)/kernels.o $(SRC)/topk.o $(SRC)/stft.o $(SRC)/mbrow.o $(SRC)/gemm_dma.o $(SRC)/gemm_dma3.o $(SRC)/gemm_b3.o $(SRC)/mbmap.o $(SRC)/mbmap_ws.o $(SRC)/index.o $(SRC)/head.o $(SRC)/rank.o $(SRC)/cluster.o $(SRC)/ivf.o $(SRC)/sq8.o $(SRC)/subset.o $(SRC)/index_copy.o $(SRC)/peaks.o $(SRC)/seq.o $(SRC)/above.o $(SRC)/group_above.o $(SRC)/match.o $(SRC)/index_io.o $(SRC)/index_file.o $(SRC)/prior.o $(SRC)/track.o $(SRC)/live.o $(SRC)/live_kernels.o $(SRC)/levels.o $(SRC)/band_levels.o

all: $(OUT) oracle

$(SRC)/%.o: $(SRC)/%.cpp $(wildcard $(SRC)/*.h) include/birdnet_hip.h include/birdnet_host.h
	$(CXX) $(CXXFLAGS) -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -c $< -o $@
$(SRC)/%.o: $(SRC)/%.hip $(wildcard $(SRC)/*.h)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
# live.cpp (host side of the live pool) and live.hip (its kernels) share a stem
$(SRC)/live_kernels.o: $(SRC)/live.hip $(wildcard $(SRC)/*.h)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
# group.cpp (the multi-GPU bn_group_*) and group.hip (the grouped threshold search, bn_index_group_above) share a stem
$(SRC)/group_above.o: $(SRC)/group.hip $(wildcard $(SRC)/*.h)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OUT): $(OBJS)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $(OBJS) -lpthread -ldl

oracle:
	$(MAKE) -C oracle

# diagnostic build: the LDS-DMA GEMM with shader-clock stamps around every K step of one block (tools/gemm_stamps.cpp; never linked into the library)
stamps: $(OUT)
	$(HIPCC) $(HIPFLAGS) -DBN_GD_STAMPS -c $(SRC)/gemm_dma.hip -o /tmp/bn_gd_stamps.o
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) -Iinclude -I$(SRC) -c tools/gemm_stamps.cpp -o /tmp/bn_gemm_stamps_main.o
	$(HIPCC) --offload-arch=$(ARCH) /tmp/bn_gemm_stamps_main.o /tmp/bn_gd_stamps.o $(SRC)/kernels.o $(SRC)/stft.o $(SRC)/topk.o $(SRC)/mbrow.o $(SRC)/mbmap.o $(SRC)/mbmap_ws.o -o tools/gemm_stamps -lpthread -ldl

# diagnostic: exact-f32 LDS-DMA GEMM against the bf16x3 form, timing + error against a double-precision product (never linked into the library)
tools/gemm3_bench: tools/gemm3_bench.cpp $(OUT)
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) -Iinclude -I$(SRC) -c tools/gemm3_bench.cpp -o /tmp/bn_gemm3_bench_main.o
	$(HIPCC) --offload-arch=$(ARCH) /tmp/bn_gemm3_bench_main.o $(SRC)/kernels.o $(SRC)/stft.o $(SRC)/topk.o $(SRC)/mbrow.o $(SRC)/mbmap.o $(SRC)/mbmap_ws.o $(SRC)/gemm_dma.o $(SRC)/gemm_dma3.o $(SRC)/gemm_b3.o -o tools/gemm3_bench -lpthread -ldl

# host-only sanitizer checks of the threshold searches', the row copy's and the sequence search's argument and plan arithmetic, and of
# the query source and round arithmetic every search over an index shares (no device)
ASAN_FLAGS := -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -I$(SRC)
tools/asan_above_plan: tools/asan_above_plan.cpp $(SRC)/above_plan.h $(SRC)/last_error.h
	$(CXX) $(ASAN_FLAGS) $< -o $@
tools/asan_query_source: tools/asan_query_source.cpp $(SRC)/query_source.h $(SRC)/last_error.h
	$(CXX) $(ASAN_FLAGS) $< -o $@
tools/asan_group_plan: tools/asan_group_plan.cpp $(SRC)/group_plan.h $(SRC)/above_plan.h $(SRC)/last_error.h
	$(CXX) $(ASAN_FLAGS) $< -o $@
tools/asan_index_copy_plan: tools/asan_index_copy_plan.cpp $(SRC)/index_copy_plan.h $(SRC)/last_error.h
	$(CXX) $(ASAN_FLAGS) $< -o $@
tools/asan_seq_plan: tools/asan_seq_plan.cpp $(SRC)/seq_plan.h $(SRC)/last_error.h
	$(CXX) $(ASAN_FLAGS) $< -o $@
# ... of the frame and byte arithmetic of the PCM layouts (offsets, upload chunks cut at frame boundaries, overflow refusals)
tools/asan_pcm_layout: tools/asan_pcm_layout.cpp $(SRC)/pcm_layout.h include/birdnet_hip.h
	$(CXX) $(ASAN_FLAGS) $< -o $@
# ... of the window list's arithmetic: frames read without forming start + S, grouping by reader kind, the 128-row launch cuts
tools/asan_window_list_plan: tools/asan_window_list_plan.cpp $(SRC)/window_list_plan.h $(SRC)/pcm_layout.h $(SRC)/last_error.h include/birdnet_hip.h
	$(CXX) $(ASAN_FLAGS) $< -o $@
# ... of the band levels' arithmetic: spec refusals, frames and the unread tail, the last sample a range reads, bins of a band in hertz, the tables
tools/asan_band_plan: tools/asan_band_plan.cpp $(SRC)/band_plan.h $(SRC)/last_error.h include/birdnet_hip.h
	$(CXX) $(ASAN_FLAGS) $< -o $@
# ... and of the operands of finished plans: the planner's own files, as tools/asan_plan.cpp links them
PLANNER_SRC := $(SRC)/onnx_proto.cpp $(SRC)/engine.cpp $(SRC)/onnx_rewrite.cpp $(SRC)/dft_bank.cpp $(SRC)/mbconv_fuse.cpp $(SRC)/plan_passes.cpp $(SRC)/detect.cpp
tools/asan_plan_operands: tools/asan_plan_operands.cpp $(PLANNER_SRC) $(wildcard $(SRC)/*.h)
	$(CXX) $(ASAN_FLAGS) -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include $< $(PLANNER_SRC) -o $@

clean:
	rm -f $(OBJS) $(OUT)
	$(MAKE) -C oracle clean
.PHONY: all oracle clean stamps
