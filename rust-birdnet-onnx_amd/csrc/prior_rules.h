// The per-species rules of a site prior (include/birdnet_hip.h, bn_prior_*), shared by the kernels that apply one: prior.hip's
// select / filter kernels and track.hip's tracker under BN_TRACK_PRIOR.  Device code only; every translation unit that includes it
// must be compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace bn {
namespace {

__device__ __forceinline__ bool admitted(float p, float thr) { return p < 0.0f || p >= thr; }
// conf' of the contract: one f32 multiply when reranking a known species
__device__ __forceinline__ float prior_conf(float conf, float p, int rerank) { return (rerank && p >= 0.0f) ? conf * p : conf; }

}  // namespace
}  // namespace bn
