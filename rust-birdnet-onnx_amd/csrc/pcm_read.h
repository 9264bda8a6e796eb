// The sample read of every kernel that takes PCM (kernels.hip: windows, resampler; live.hip: scatter, streaming resampler, history):
// frame index -> the f32 sample the layout rule defines (include/birdnet_hip.h, "PCM layouts").  A kernel is a template over a
// reader and calls rd(i); pcm_visit() picks the reader for a PcmSrc on the host.
//
//   PcmMono<int16_t> / PcmMono<float>  mono int16 / float: the loads these kernels always had (v / 32768, or the float as is)
//   PcmFrames<FORMAT>                  interleaved frames of any format; `channel` selects or, at BN_PCM_MIX, mixes:
//                                      acc = s[0]; acc = acc + s[c] for c = 1, 2, ...; acc * inv, inv = 1.0f / channels rounded once
//                                      on the host.  Plain f32 operations in that order (the library is built with
//                                      -ffp-contract=off: no multiply-add is fused anywhere in it).
//
// Loads.  Neighbouring lanes of the callers read neighbouring frames, so a wave's loads cover one contiguous span of the
// storage.  I16, I32, F32 and U8 samples are naturally aligned loads of their own width.  A packed I24 sample is read from the
// aligned dword that holds its first byte, and from the next one only when the sample crosses into it, then shifted into place in
// registers -- never three byte loads.  That dword may reach up to 3 bytes past the last sample: buffers carry PCM_READ_SLACK.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcm_layout.h"

namespace bn {

template <class T>
struct PcmMono {
    const T *p;
    __device__ __forceinline__ float operator()(uint64_t i) const {
        if constexpr (sizeof(T) == 2) return (float)p[i] * (1.0f / 32768.0f);
        else return (float)p[i];
    }
    __device__ __forceinline__ PcmMono from(uint64_t first) const { return PcmMono{p + first}; }
};

template <int FORMAT>
__device__ __forceinline__ float pcm_sample(const uint8_t *p, uint64_t k) {
    if constexpr (FORMAT == BN_PCM_I16) {
        return (float)reinterpret_cast<const int16_t *>(p)[k] * (1.0f / 32768.0f);
    } else if constexpr (FORMAT == BN_PCM_F32) {
        return reinterpret_cast<const float *>(p)[k];
    } else if constexpr (FORMAT == BN_PCM_I32) {
        return (float)reinterpret_cast<const int32_t *>(p)[k] * 4.656612873077392578125e-10f;  // round to nearest even, then * 2^-31
    } else if constexpr (FORMAT == BN_PCM_U8) {
        return (float)((int32_t)p[k] - 128) * (1.0f / 128.0f);
    } else {
        static_assert(FORMAT == BN_PCM_I24, "unknown PCM format");
        const uint64_t a = reinterpret_cast<uint64_t>(p) + 3u * k;
        const uint32_t *w = reinterpret_cast<const uint32_t *>(a & ~(uint64_t)3);
        const uint32_t ph = (uint32_t)a & 3u;
        uint32_t bits = w[0] >> (8u * ph);
        if (ph >= 2u) bits |= w[1] << (32u - 8u * ph);
        return (float)((int32_t)(bits << 8) >> 8) * (1.0f / 8388608.0f);
    }
}

template <int FORMAT>
struct PcmFrames {
    const uint8_t *p;   // first byte of frame 0
    uint32_t channels;  // 1..16
    int32_t channel;    // in [0, channels), or BN_PCM_MIX
    float inv;          // 1.0f / channels
    __device__ __forceinline__ float operator()(uint64_t i) const {
        const uint64_t k = i * channels;
        if (channel >= 0) return pcm_sample<FORMAT>(p, k + (uint32_t)channel);
        float acc = pcm_sample<FORMAT>(p, k);
        for (uint32_t c = 1; c < channels; c++) acc = acc + pcm_sample<FORMAT>(p, k + c);
        return acc * inv;
    }
    __device__ __forceinline__ PcmFrames from(uint64_t first) const {
        return PcmFrames{p + first * channels * (FORMAT == BN_PCM_I24 ? 3u : FORMAT == BN_PCM_U8 ? 1u : FORMAT == BN_PCM_I16 ? 2u : 4u), channels, channel, inv};
    }
};

// f(reader) for the reader of `s` (its layout checked and normalised by the caller); false for a format no reader knows
template <class F>
inline bool pcm_visit(const PcmSrc &s, F &&f) {
    const PcmLayout &l = s.layout;
    if (pcm_is_plain(l)) {
        if (l.format == BN_PCM_I16) f(PcmMono<int16_t>{static_cast<const int16_t *>(s.base)});
        else f(PcmMono<float>{static_cast<const float *>(s.base)});
        return true;
    }
    const uint8_t *p = static_cast<const uint8_t *>(s.base);
    const float inv = 1.0f / (float)l.channels;
    switch (l.format) {
        case BN_PCM_I16: f(PcmFrames<BN_PCM_I16>{p, l.channels, l.channel, inv}); return true;
        case BN_PCM_F32: f(PcmFrames<BN_PCM_F32>{p, l.channels, l.channel, inv}); return true;
        case BN_PCM_I24: f(PcmFrames<BN_PCM_I24>{p, l.channels, l.channel, inv}); return true;
        case BN_PCM_I32: f(PcmFrames<BN_PCM_I32>{p, l.channels, l.channel, inv}); return true;
        case BN_PCM_U8: f(PcmFrames<BN_PCM_U8>{p, l.channels, l.channel, inv}); return true;
        default: return false;
    }
}

}  // namespace bn
