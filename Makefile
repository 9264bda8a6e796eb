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
OBJS := $(SRC)/onnx_proto.o $(SRC)/engine.o $(SRC)/onnx_rewrite.o $(SRC)/dft_bank.o $(SRC)/mbconv_fuse.o $(SRC)/plan_passes.o $(SRC)/detect.o $(SRC)/capi.o $(SRC)/recording.o $(SRC)/step_common.o $(SRC)/group.o $(SRC)/host_classifier.o $(SRC)/host_capi.o $(SRC)/host_rangefilter.o $(SRC)/kernels.o $(SRC)/topk.o $(SRC)/stft.o $(SRC)/mbrow.o $(SRC)/gemm_dma.o $(SRC)/gemm_dma3.o $(SRC)/gemm_b3.o $(SRC)/mbmap.o $(SRC)/mbmap_ws.o $(SRC)/index.o $(SRC)/head.o $(SRC)/rank.o $(SRC)/cluster.o $(SRC)/ivf.o $(SRC)/sq8.o $(SRC)/subset.o $(SRC)/index_copy.o $(SRC)/peaks.o $(SRC)/seq.o $(SRC)/above.o $(SRC)/group_above.o $(SRC)/match.o $(SRC)/index_io.o $(SRC)/index_file.o $(SRC)/prior.o $(SRC)/track.o $(SRC)/live.o $(SRC)/live_kernels.o $(SRC)/levels.o $(SRC)/band_levels.o $(SRC)/spectral_profile.o $(SRC)/fir.o $(SRC)/denoise.o $(SRC)/spectrogram.o $(SRC)/delay.o $(SRC)/template.o $(SRC)/pcen.o

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
# fir.hip: packed f32 instructions are switched off for the device code outright (nothing in it gains from them; the split of a sample
# pair is what the vectorizers would otherwise pair up)
$(SRC)/fir.o: $(SRC)/fir.hip $(wildcard $(SRC)/*.h)
	$(HIPCC) $(HIPFLAGS) -Xclang -target-feature -Xclang -packed-fp32-ops -c $< -o $@
# spectral_profile.hip: the same switch (scalar f32 chains whose order is the contract; nothing to pack)
$(SRC)/spectral_profile.o: $(SRC)/spectral_profile.hip $(wildcard $(SRC)/*.h)
	$(HIPCC) $(HIPFLAGS) -Xclang -target-feature -Xclang -packed-fp32-ops -c $< -o $@
# denoise.hip: the same switch (plain f32 butterflies whose bits are the contract)
$(SRC)/denoise.o: $(SRC)/denoise.hip $(wildcard $(SRC)/*.h)
	$(HIPCC) $(HIPFLAGS) -Xclang -target-feature -Xclang -packed-fp32-ops -c $< -o $@
# spectrogram.hip: the same switch (band levels' transform and the split of a power pair)
$(SRC)/spectrogram.o: $(SRC)/spectrogram.hip $(wildcard $(SRC)/*.h)
	$(HIPCC) $(HIPFLAGS) -Xclang -target-feature -Xclang -packed-fp32-ops -c $< -o $@
# delay.hip: the same switch (scalar f32 chains whose order is the contract)
$(SRC)/delay.o: $(SRC)/delay.hip $(wildcard $(SRC)/*.h)
	$(HIPCC) $(HIPFLAGS) -Xclang -target-feature -Xclang -packed-fp32-ops -c $< -o $@
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
# ... of the spectral profile's arithmetic: spec refusals, each wave's run of frames and its boundary frame, the LDS swizzle, the size of the planes
tools/asan_profile_plan: tools/asan_profile_plan.cpp $(SRC)/profile_plan.h $(SRC)/band_plan.h $(SRC)/last_error.h include/birdnet_hip.h
	$(CXX) $(ASAN_FLAGS) $< -o $@
# ... of the delay estimate's arithmetic: spec refusals, Z of both weightings, every LDS position the kernel touches, the lag row, the
# peak key against the tie rule, the curve's sizes, bn_delay_refine
tools/asan_delay_plan: tools/asan_delay_plan.cpp $(SRC)/delay_plan.h $(SRC)/profile_plan.h $(SRC)/band_plan.h $(SRC)/last_error.h include/birdnet_hip.h
	$(CXX) $(ASAN_FLAGS) $< -o $@
# ... of template matching's arithmetic: the caps, the output and image sizes at extreme n_offsets, the launch pieces and their overlap, the
# packed templates against a direct index formula with T1 and dT, the B operand's walk through LDS, bn_template_peaks
tools/asan_template_plan: tools/asan_template_plan.cpp $(SRC)/template_plan.h $(SRC)/spectrogram_plan.h $(SRC)/band_plan.h $(SRC)/plan_rules.h $(SRC)/last_error.h include/birdnet_hip.h
	$(CXX) $(ASAN_FLAGS) -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include $< -o $@
# ... of the noise reduction's arithmetic: spec and noise refusals, every (frame, register, lane) position the kernel reads or stores for
# ragged lengths, the register shift, the window table, bn_noise_floor's selection
tools/asan_denoise_plan: tools/asan_denoise_plan.cpp $(SRC)/denoise_plan.h $(SRC)/band_plan.h $(SRC)/last_error.h include/birdnet_hip.h
	$(CXX) $(ASAN_FLAGS) $< -o $@
# ... of the FIR filter's arithmetic: tap refusals, the designer, the chunk geometry, the packed Toeplitz operand (plan_rules.h's split
# needs the runtime's headers, no more)
tools/asan_fir_plan: tools/asan_fir_plan.cpp $(SRC)/fir_plan.h $(SRC)/plan_rules.h $(SRC)/last_error.h include/birdnet_hip.h
	$(CXX) $(ASAN_FLAGS) -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include $< -o $@
# ... of the spectrogram's arithmetic: spec, bank and designer refusals, sizes and starts at extreme n_frames and hop, the LDS strides,
# the packed bank re-summed to its weights with each tile's step range, the threshold table
tools/asan_spectrogram_plan: tools/asan_spectrogram_plan.cpp $(SRC)/spectrogram_plan.h $(SRC)/band_plan.h $(SRC)/plan_rules.h $(SRC)/last_error.h include/birdnet_hip.h
	$(CXX) $(ASAN_FLAGS) -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include $< -o $@
# ... of PCEN's arithmetic: the spec's refusals field by field, bytes formed without wrapping, the launch pieces at a small piece length with
# every chunk's start and the last partial chunk, apow against a running product, the threshold table
tools/asan_pcen_plan: tools/asan_pcen_plan.cpp $(SRC)/pcen_plan.h $(SRC)/spectrogram_plan.h $(SRC)/band_plan.h $(SRC)/plan_rules.h $(SRC)/last_error.h include/birdnet_hip.h
	$(CXX) $(ASAN_FLAGS) -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include $< -o $@
# ... and of the operands of finished plans: the planner's own files, as tools/asan_plan.cpp links them
PLANNER_SRC := $(SRC)/onnx_proto.cpp $(SRC)/engine.cpp $(SRC)/onnx_rewrite.cpp $(SRC)/dft_bank.cpp $(SRC)/mbconv_fuse.cpp $(SRC)/plan_passes.cpp $(SRC)/detect.cpp
tools/asan_plan_operands: tools/asan_plan_operands.cpp $(PLANNER_SRC) $(wildcard $(SRC)/*.h)
	$(CXX) $(ASAN_FLAGS) -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include $< $(PLANNER_SRC) -o $@

clean:
	rm -f $(OBJS) $(OUT)
	$(MAKE) -C oracle clean
.PHONY: all oracle clean stamps
