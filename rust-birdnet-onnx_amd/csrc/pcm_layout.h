// PCM layouts (include/birdnet_hip.h, "PCM layouts"): all arithmetic on frames and bytes of interleaved PCM, in one place and in
// plain C++ -- the recording upload (recording.cpp), the live pool (live.cpp) and the kernels' sample read (pcm_read.h) take their
// offsets, chunk cuts and sizes from here, and tools/asan_pcm_layout.cpp runs it under the sanitizers without a device.
//
// A layout is {format, channels, channel}: frames of `channels` samples, each pcm_sample_bytes(format) wide, little-endian;
// channel >= 0 selects one sample of the frame, BN_PCM_MIX (-1) mixes the frame down.  Counts are FRAMES everywhere.
#pragma once
#include <cstddef>
#include <cstdint>

#include "birdnet_hip.h"

namespace bn {

constexpr uint32_t PCM_MAX_CHANNELS = 16;

struct PcmLayout {
    int32_t format = BN_PCM_I16;
    uint32_t channels = 1;
    int32_t channel = 0;
};

// what a kernel reads: the layout and the first byte of frame 0
struct PcmSrc {
    const void *base = nullptr;
    PcmLayout layout;
};

// bytes of one stored sample; 0 for a format the library does not know
inline uint32_t pcm_sample_bytes(int32_t format) {
    switch (format) {
        case BN_PCM_I16: return 2;
        case BN_PCM_F32: return 4;
        case BN_PCM_I24: return 3;
        case BN_PCM_I32: return 4;
        case BN_PCM_U8: return 1;
        default: return 0;
    }
}

// nullptr for a layout the library accepts, else what is wrong with it
inline const char *pcm_layout_problem(const PcmLayout &l) {
    if (pcm_sample_bytes(l.format) == 0) return "unknown PCM format";
    if (l.channels < 1 || l.channels > PCM_MAX_CHANNELS) return "channels must be in 1..16";
    if (l.channel < BN_PCM_MIX || (l.channel >= 0 && (uint32_t)l.channel >= l.channels)) return "channel must be BN_PCM_MIX or in [0, channels)";
    return nullptr;
}

// one channel is its own mix: both ops are the identity there, and the select form keeps the stored bits (a NaN's payload)
inline PcmLayout pcm_normalised(PcmLayout l) {
    if (l.channels == 1) l.channel = 0;
    return l;
}

// mono int16 / float: the layouts the library always took, served by the loads it always used
inline bool pcm_is_plain(const PcmLayout &l) { return l.channels == 1 && (l.format == BN_PCM_I16 || l.format == BN_PCM_F32); }

inline size_t pcm_frame_bytes(const PcmLayout &l) { return (size_t)pcm_sample_bytes(l.format) * l.channels; }

// bytes of n_frames frames; false when the product does not fit size_t (nothing is written then)
inline bool pcm_bytes(const PcmLayout &l, size_t n_frames, size_t *out) {
    const size_t fb = pcm_frame_bytes(l);
    if (fb == 0 || n_frames > SIZE_MAX / fb) return false;
    *out = n_frames * fb;
    return true;
}

// byte offset of frame i (the caller has checked pcm_bytes for a count above i)
inline size_t pcm_frame_offset(const PcmLayout &l, size_t i) { return i * pcm_frame_bytes(l); }

// byte offset of the sample channel c of frame i
inline size_t pcm_sample_offset(const PcmLayout &l, size_t i, uint32_t c) { return i * pcm_frame_bytes(l) + (size_t)c * pcm_sample_bytes(l.format); }

// frames per chunk of the asynchronous upload: the largest whole number of frames within chunk_bytes, at least one -- a chunk ends
// on a frame boundary, whatever the frame's size (6 bytes do not divide 32 MiB)
inline size_t pcm_chunk_frames(const PcmLayout &l, size_t chunk_bytes) {
    const size_t n = chunk_bytes / pcm_frame_bytes(l);
    return n ? n : 1;
}

inline size_t pcm_chunk_count(size_t n_frames, size_t chunk_frames) { return n_frames / chunk_frames + (n_frames % chunk_frames != 0); }

// chunks that must have landed before frame `last` is on the device
inline size_t pcm_chunks_for_frame(size_t last, size_t chunk_frames, size_t n_chunks) {
    const size_t k = last / chunk_frames;
    return (k < n_chunks - 1 ? k : n_chunks - 1) + 1;
}

// bytes of a live pool's slab: n_sources rings of ring_samples elements of elem_bytes; false on overflow
inline bool pcm_ring_bytes(size_t n_sources, size_t ring_samples, size_t elem_bytes, size_t *out) {
    if (elem_bytes == 0 || n_sources == 0) return false;
    if (ring_samples > SIZE_MAX / elem_bytes) return false;
    const size_t one = ring_samples * elem_bytes;
    if (one > SIZE_MAX / n_sources) return false;
    *out = one * n_sources;
    return true;
}

// the kernels read I24 through the aligned dwords that hold it: the last sample's dword may end up to 3 bytes past the data, so
// every buffer a kernel reads samples from is allocated with this much behind it
constexpr size_t PCM_READ_SLACK = 4;

}  // namespace bn
