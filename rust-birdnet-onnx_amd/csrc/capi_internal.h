// What other translation units of the C ABI need of capi.cpp's private state (index.hip: bn_index_*).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

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
}  // namespace bn
