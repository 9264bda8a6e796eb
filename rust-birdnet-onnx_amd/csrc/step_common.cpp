// The plumbing the entry points of the C ABI share (declared in capi_internal.h): launch and device checks, the packed top-K block,
// results to pinned memory, the pinned ring, scoped scratch.
#include <algorithm>

#include "capi_internal.h"
#include "kernels.h"

namespace bn {

void clear_launch_state() {
    (void)take_launch_error();
    (void)hipGetLastError();
}

bn_status check_launch(const char *what) {
    if (const char *why = take_launch_error()) return set_last_error(BN_ERR_INVALID_ARG, std::string(what) + " refused: " + why);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_last_error(BN_ERR_BACKEND, std::string(what) + " launch failed: " + hipGetErrorString(e));
    return BN_OK;
}

bn_status require_any_device() {
    if (bn_device_count() <= 0) return set_last_error(BN_ERR_NO_DEVICE, "no gfx950 device visible");
    return BN_OK;
}

bn_status require_device(int32_t device) {
    bn_status st = require_any_device();
    if (st != BN_OK) return st;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return set_last_error(BN_ERR_NO_DEVICE, "no such device");
    return BN_OK;
}

bn_status check_top_k(size_t n, size_t top_k, size_t *k) {
    *k = std::min(top_k, n);
    if (*k == 0 || topk_lds_bytes((int64_t)n, (int64_t)*k) == 0)
        return set_last_error(BN_ERR_INVALID_ARG, "top_k must be in 1..9000, got " + std::to_string(top_k));
    return BN_OK;
}

bn_status TopkRows::reserve(size_t max_batch, size_t k, hipStream_t drain, bool device, bool pinned) {
    const size_t need = words(max_batch, k);
    if (need <= cap) return BN_OK;
    if (drain) BN_HIP_TRY(hipStreamSynchronize(drain));  // the last step may still write the old blocks
    release();
    hipError_t e = device ? d.alloc(need * sizeof(uint32_t)) : hipSuccess;
    if (e == hipSuccess && pinned) e = h.alloc(need * sizeof(uint32_t));
    if (e != hipSuccess) {
        release();
        return set_last_error(BN_ERR_BACKEND, std::string("allocating the top-K rows failed: ") + hipGetErrorString(e));
    }
    cap = need;
    return BN_OK;
}

void TopkRows::release() {
    d.reset();
    h.reset();
    cap = last_batch = last_k = 0;
}

bn_status TopkRows::results(const char *none_msg, const uint32_t **idx, const float **conf, const uint32_t **count, size_t *k_stride) const {
    if (!h || last_k == 0) return set_last_error(BN_ERR_INVALID_ARG, none_msg);
    const ConstView v = view(static_cast<const uint32_t *>(h), last_batch, last_k);
    if (idx) *idx = v.idx;
    if (conf) *conf = v.conf;
    if (count) *count = v.count;
    if (k_stride) *k_stride = v.k;
    return BN_OK;
}

// BN_SDMA_COPY=1 restores the hipMemcpyAsync transfers (A/B measurements); they also serve whatever the kernel cannot take: more than
// three regions, a size that is no multiple of 4 bytes, host memory the device cannot address
bn_status results_to_host(hipStream_t stream, const OutRegion *regs, int n) {
    static const bool sdma = sw_int(sw::BN_SDMA_COPY) != 0;
    CopyOut co{};
    bool kernel_ok = !sdma && n <= 3;
    for (int r = 0; r < n && kernel_ok; r++) {
        void *dp = nullptr;
        if (regs[r].bytes % 4 || regs[r].bytes / 4 > 0xffffffffull || hipHostGetDevicePointer(&dp, regs[r].host, 0) != hipSuccess || !dp) {
            (void)hipGetLastError();
            kernel_ok = false;
            break;
        }
        co.dst[r] = dp;
        co.src[r] = regs[r].dev;
        co.words[r] = (uint32_t)(regs[r].bytes / 4);
    }
    if (kernel_ok) {
        co.n = n;
        launch_copy_out(stream, co);
        return check_launch("results to host");
    }
    for (int r = 0; r < n; r++)
        if (regs[r].bytes) BN_HIP_TRY(hipMemcpyAsync(regs[r].host, regs[r].dev, regs[r].bytes, hipMemcpyDeviceToHost, stream));
    return BN_OK;
}

bn_status enqueue_topk_rows(hipStream_t stream, const float *d_logits, size_t rows, size_t n, size_t k, int32_t has_min, float min_conf,
                            const TopkRows::View &out, uint32_t *d_flags) {
    clear_launch_state();
    launch_topk(stream, d_logits, (int64_t)rows, (int64_t)n, (int64_t)k, has_min, min_conf, (int64_t)k, out.idx, out.conf, out.count, d_flags);
    return check_launch("top-K");
}

hipError_t PinnedRing::create(size_t bytes) {
    hipError_t e = hipSuccess;
    for (int i = 0; i < SLOTS && e == hipSuccess; i++) {
        e = h[i].alloc(bytes);
        if (e == hipSuccess) e = hipHostGetDevicePointer(&d[i], h[i], 0);
        if (e == hipSuccess) e = ev[i].create(hipEventDisableTiming);
    }
    if (e != hipSuccess) release();
    return e;
}

void PinnedRing::release() { *this = PinnedRing{}; }

hipError_t PinnedRing::acquire(int *slot, void **host) {
    if (busy[next]) {
        hipError_t e = hipEventSynchronize(ev[next]);
        if (e != hipSuccess) return e;
    }
    *slot = next;
    *host = h[next];
    return hipSuccess;
}

hipError_t PinnedRing::commit(int slot, hipStream_t stream) {
    hipError_t e = hipEventRecord(ev[slot], stream);
    if (e != hipSuccess) return e;
    busy[slot] = true;
    next = (slot + 1) % SLOTS;
    return hipSuccess;
}

}  // namespace bn
