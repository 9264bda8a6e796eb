// The digest of the index file format (include/birdnet_hip.h, bn_index_save): defined once, in plain C++, for the host
// (index_file.cpp) and for the kernels (index_io.hip).  Element `u` of a stream (for the payload u = row id * dim + component, for the
// header u = the word's number) with 32-bit value `b` contributes digest_term(u, b); a digest is the sum of its terms mod 2^64, so
// the terms may be added in any order and partial sums (threads, waves, blocks, slices of a chunk) compose.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define BN_DIGEST_FN __host__ __device__ inline
#else
#define BN_DIGEST_FN inline
#endif

namespace bn {
BN_DIGEST_FN uint64_t digest_term(uint64_t u, uint32_t b) {
    uint64_t z = u * 0x9E3779B97F4A7C15ull + b;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// a row of the file is invalid exactly when every element is +0.0 or -0.0
BN_DIGEST_FN bool digest_is_zero(uint32_t b) { return (b & 0x7fffffffu) == 0; }
BN_DIGEST_FN bool digest_is_finite(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }
}  // namespace bn
