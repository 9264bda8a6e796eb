// What other translation units of the C ABI need of capi.cpp's private state (index.hip: bn_index_*; head.hip: bn_head_*) and
// of each other (prior.hip: bn_prior_*).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/birdnet_hip.h"

namespace bn {
// sets the message bn_last_error() returns on this thread; returns st
bn_status set_last_error(bn_status st, const std::string &msg);
// the embedding output of a context's last run: device, stream, rows [last_batch, row_elems]; BN_ERR_INVALID_ARG (message set)
// for a model without embeddings
struct CtxEmbedding {
    int device = 0;
    hipStream_t stream = nullptr;
    const float *d_rows = nullptr;
    size_t row_elems = 0;
    size_t last_batch = 0;
};
bn_status ctx_embedding(const bn_ctx *c, CtxEmbedding *out);
// what bn_step_live needs of a context: its device, stream and input buffer [max_batch, sample_count]; BN_ERR_INVALID_ARG
// (message set) for a top_k that bn_step_device would refuse
struct CtxStepInput {
    int device = 0;
    hipStream_t stream = nullptr;
    float *d_input = nullptr;
    size_t sample_count = 0;
    size_t max_batch = 0;
};
bn_status ctx_step_input(const bn_ctx *c, size_t top_k, CtxStepInput *out);
// the polyphase table of the resampler (design in include/birdnet_hip.h): L/M = dst/src reduced, T taps per phase; zc 0 => 16
struct ResampleTable {
    uint32_t L = 1, M = 1, T = 0;
    std::vector<float> coef;  // [L][T]
};
// L, M and T alone (coef left empty): what the table would be, without building it
ResampleTable resample_factors(uint32_t src_rate, uint32_t dst_rate, uint32_t zc);
ResampleTable make_resample_table(uint32_t src_rate, uint32_t dst_rate, uint32_t zc);
// index.hip -> head.hip (bn_head_fit_index): the stored rows of an index, every pending append waited for
struct IndexRows {
    int device = 0;
    const float *slab = nullptr;   // [size, dpad], rows normalised, zero-padded to dpad (a multiple of 128)
    const uint8_t *valid = nullptr;  // [size]: 0 for a row stored as zeros
    size_t dim = 0, dpad = 0, size = 0;
};
bn_status index_rows(bn_index *x, IndexRows *out);
// head.hip -> capi.cpp: a head attached to a context (its own result buffers; holds a reference to the head)
struct HeadAttach;
bn_status head_attach(bn_head *h, int device, bool has_embedding, size_t embedding_dim, size_t max_batch, size_t top_k, int32_t has_min,
                      float min_conf, HeadAttach **out);
void head_detach(HeadAttach *a);  // the context's stream must be idle
// prep + apply + top-K + results to pinned memory, enqueued on the context's stream behind the step's own work
bn_status head_step(HeadAttach *a, hipStream_t stream, const float *d_emb, size_t batch);
bn_status head_step_results(const HeadAttach *a, const float **logits, const uint32_t **idx, const float **conf, const uint32_t **count,
                            size_t *k_stride, size_t *n_classes);
// prior.hip -> capi.cpp / live.cpp: a prior attached to a context (its own result buffers; holds a reference to the prior)
struct PriorAttach;
bn_status prior_attach(bn_prior *p, int device, size_t num_species, size_t max_batch, const int32_t *source_sites, size_t n_source_sites, size_t top_k,
                       int32_t has_min, float min_conf, PriorAttach **out);
void prior_detach(PriorAttach *a);  // the context's stream must be idle
bn_status prior_set_site(PriorAttach *a, int32_t site);
// bn_step_live: refuses a pool with more sources than the attached map, before anything is taken from the pool
bn_status prior_live_check(const PriorAttach *a, size_t n_sources);
// bn_step_live: the sites of the coming step's rows (by source) into the next pinned block; prior_step consumes it
bn_status prior_stage_rows(PriorAttach *a, const int32_t *sources, size_t rows);
void prior_clear_rows(PriorAttach *a);
// the prior kernel + results to pinned memory, enqueued on the context's stream behind the step's own top-K;
// d_step_rows / step_k: the step's packed [idx][conf][count] block on the device
bn_status prior_step(PriorAttach *a, hipStream_t stream, const float *d_logits, size_t batch, const uint32_t *d_step_rows, size_t step_k);
bn_status prior_step_results(const PriorAttach *a, const uint32_t **idx, const float **conf, const uint32_t **count, size_t *k_stride);
// capi.cpp -> live.cpp: the context's attached prior, NULL if none
PriorAttach *ctx_prior(bn_ctx *c);
}  // namespace bn
