// Per-site species priors on the device (include/birdnet_hip.h, bn_prior_*): the location / date prior of the reference's
// RangeFilter (src/rangefilter.rs:333-386) as a table P[site][species], applied to every row of a step.
//
// Two kernels, one block of 256 threads per logits row.
//
// prior_select_kernel (BN_PRIOR_SELECT): the K best ADMITTED species of the row, which needs the prior in front of the
// selection, over all n logits.
//   1  keys    16-byte loads of the logits row and of the site's table row (rows that share a site hit L2);
//              conf' = sigmoid_ref(z) [* p], key = total_cmp key of conf' for an admitted species, 0 for any other.  The
//              keys stay in dynamic LDS (n <= 16384: 64 KB) or, in the general form, in a global scratch row that only
//              this block touches.  The admitted species are counted: K' = min(K, admitted).
//   2  select  the K'-th largest key T by an 8-bit-digit radix select: four histogram passes (integer LDS atomics: the
//              counts do not depend on their order), each followed by one block scan over the 256 bins.  A species that
//              is not admitted can only be counted where T == 0, and key 0 belongs to an admitted species only when
//              conf' is the NaN with every bit set; pass 3 then asks the table again for the entries with key 0.
//   3  compact every thread owns a contiguous range of the row; one block scan gives the keys above T their slots in
//              index order and the ties at T theirs, of which the first K' - (number above T) are taken: ascending index.
//   4  sort    rank sort of the <= 1024 survivors by (key descending, index ascending), the minimum-confidence cut by one
//              more scan, rows packed as the step's own top-K rows are.
// No floating-point atomics, no order that depends on scheduling: the result is a function of the row, its site's table
// row and the parameters alone.
//
// prior_after_kernel (BN_PRIOR_AFTER_TOPK): filter_predictions over the step's packed top-K row, species matched by
// index: drop what is not admitted, multiply when reranking, stable descending total_cmp sort when reranking.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "hip_gate.h"
#include "kernels.h"
#include "prior_rules.h"
#include "sigmoid_ref.h"

namespace bn {
namespace {

constexpr int PT = 256;                  // threads per block of both kernels
constexpr uint32_t SEL_K_MAX = 1024;     // survivors the select kernel sorts in LDS
constexpr int64_t SEL_LDS_MAX_N = 16384;  // longest row whose keys stay in LDS

// exclusive prefix sum of v over the block's 256 threads, and the block's total; sw: 4 words of LDS
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *sw, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= (uint32_t)d) inc += o;
    }
    __syncthreads();  // the previous scan's readers are done with sw
    if (lane == 63) sw[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < PT / 64; w++) {
        const uint32_t t = sw[w];
        base += w < wave ? t : 0u;
        total += t;
    }
    return base + inc - v;
}

// four consecutive floats from an address that is only known to be 4-byte aligned; the branch is the same for every lane of
// a launch's row (lanes are 16 bytes apart)
__device__ __forceinline__ float4 load4(const float *p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if ((a & 15u) == 0) return *reinterpret_cast<const float4 *>(p);
    if ((a & 7u) == 0) {
        const float2 u = *reinterpret_cast<const float2 *>(p), v = *reinterpret_cast<const float2 *>(p + 2);
        return make_float4(u.x, u.y, v.x, v.y);
    }
    return make_float4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ uint32_t select_key(float z, float p, float thr, int rerank, uint32_t &adm) {
    adm = admitted(p, thr) ? 1u : 0u;
    const float c = prior_conf(sigmoid_ref(z), p, rerank);
    return adm ? total_key(__float_as_uint(c)) : 0u;
}

struct SelectArgs {
    const float *logits;   // [rows, n]
    const float *table;    // [n_sites, tstride]
    const int32_t *sites;  // [rows] or NULL: every row at `site`
    uint32_t *gkeys;       // general form: [rows, n] scratch
    uint32_t *idx_out;     // [rows, k_stride]
    float *conf_out;
    uint32_t *count_out;   // [rows]
    int64_t n, tstride, k_stride;
    uint32_t n_sites, k;
    int32_t site, rerank, has_min;
    float thr, min_conf;
};

template <bool GLOBAL>
__global__ __launch_bounds__(PT) void prior_select_kernel(SelectArgs a) {
    extern __shared__ __align__(16) uint32_t dyn_keys[];
    __shared__ uint32_t ckey[SEL_K_MAX], cidx[SEL_K_MAX], skey[SEL_K_MAX], sidx[SEL_K_MAX];
    __shared__ uint32_t hist[PT];
    __shared__ uint32_t sw[4];
    __shared__ uint32_t s_digit, s_rem;

    const uint32_t tid = threadIdx.x;
    const int64_t row = blockIdx.x, n = a.n;
    uint32_t s = a.sites ? (uint32_t)a.sites[row] : (uint32_t)a.site;
    if (s >= a.n_sites) s = 0;  // the host has checked every id; never read outside the table
    const float *x = a.logits + row * n;
    const float *pr = a.table + (int64_t)s * a.tstride;
    uint32_t *keys = GLOBAL ? a.gkeys + row * n : dyn_keys;
    uint32_t *io = a.idx_out + row * a.k_stride;
    float *co = a.conf_out + row * a.k_stride;

    // ---- 1: keys ----
    const int64_t head = std::min<int64_t>(n, (int64_t)((4u - (uint32_t)((reinterpret_cast<uintptr_t>(x) >> 2) & 3u)) & 3u));
    const int64_t n4 = (n - head) >> 2;
    uint32_t n_adm = 0;
    for (int64_t g = tid; g < n4; g += PT) {
        const int64_t j = head + 4 * g;
        const float4 z = *reinterpret_cast<const float4 *>(x + j);
        const float4 p = load4(pr + j);
        uint32_t a0, a1, a2, a3;
        const uint32_t k0 = select_key(z.x, p.x, a.thr, a.rerank, a0), k1 = select_key(z.y, p.y, a.thr, a.rerank, a1);
        const uint32_t k2 = select_key(z.z, p.z, a.thr, a.rerank, a2), k3 = select_key(z.w, p.w, a.thr, a.rerank, a3);
        keys[j] = k0;
        keys[j + 1] = k1;
        keys[j + 2] = k2;
        keys[j + 3] = k3;
        n_adm += a0 + a1 + a2 + a3;
    }
    {  // the row's unaligned ends: fewer than 3 + 3 elements
        const int64_t tail0 = head + 4 * n4;
        int64_t j = -1;
        if ((int64_t)tid < head) j = tid;
        else if ((int64_t)tid - head < n - tail0) j = tail0 + ((int64_t)tid - head);
        if (j >= 0) {
            uint32_t a0;
            keys[j] = select_key(x[j], pr[j], a.thr, a.rerank, a0);
            n_adm += a0;
        }
    }
    uint32_t total_adm;
    (void)block_scan(n_adm, sw, total_adm);  // its barriers also publish the keys
    const uint32_t K = a.k;
    const uint32_t kp = std::min(K, total_adm);
    if (kp == 0) {
        for (uint32_t j = tid; j < K; j += PT) {
            io[j] = 0u;
            co[j] = 0.0f;
        }
        if (tid == 0) a.count_out[row] = 0u;
        return;
    }

    // ---- 2: the kp-th largest key, a digit at a time ----
    uint32_t prefix = 0, mask = 0, rem = kp;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0u;
        __syncthreads();
        for (int64_t i = tid; i < n; i += PT) {
            const uint32_t kk = keys[i];
            if ((kk & mask) == prefix) atomicAdd(&hist[(kk >> shift) & 255u], 1u);
        }
        __syncthreads();
        const uint32_t h = hist[tid];
        uint32_t tot;
        const uint32_t excl = block_scan(h, sw, tot);
        const uint32_t above = tot - (excl + h);  // entries in the bins over this thread's
        if (above < rem && rem <= above + h) {    // exactly one thread
            s_digit = tid;
            s_rem = rem - above;
        }
        __syncthreads();
        prefix |= s_digit << shift;
        mask |= 255u << shift;
        rem = s_rem;
        __syncthreads();
    }
    const uint32_t T = prefix;      // rem of the entries with key == T are taken, lowest index first
    const uint32_t n_above = kp - rem;

    // ---- 3: compact, in index order ----
    const int64_t per = ((n + PT - 1) / PT) | 1;  // odd: the threads' ranges start in different LDS banks
    const int64_t r0 = std::min<int64_t>(n, (int64_t)tid * per), r1 = std::min<int64_t>(n, r0 + per);
    uint32_t cg = 0, ce = 0;
    for (int64_t i = r0; i < r1; i++) {
        const uint32_t kk = keys[i];
        cg += kk > T ? 1u : 0u;
        ce += (kk == T && (T != 0u || admitted(pr[i], a.thr))) ? 1u : 0u;
    }
    uint32_t tg, te;
    uint32_t og = block_scan(cg, sw, tg);
    uint32_t oe = block_scan(ce, sw, te);
    for (int64_t i = r0; i < r1; i++) {
        const uint32_t kk = keys[i];
        if (kk > T) {
            if (og < SEL_K_MAX) {
                ckey[og] = kk;
                cidx[og] = (uint32_t)i;
            }
            og++;
        } else if (kk == T && (T != 0u || admitted(pr[i], a.thr))) {
            if (oe < rem) {
                ckey[n_above + oe] = kk;
                cidx[n_above + oe] = (uint32_t)i;
            }
            oe++;
        }
    }
    __syncthreads();

    // ---- 4: sort by (key descending, index ascending), cut, write ----
    for (uint32_t i = tid; i < kp; i += PT) {
        const uint32_t ki = ckey[i], ii = cidx[i];
        uint32_t r = 0;
        for (uint32_t j = 0; j < kp; j++) {
            const uint32_t kj = ckey[j];
            r += (kj > ki || (kj == ki && cidx[j] < ii)) ? 1u : 0u;
        }
        skey[r] = ki;
        sidx[r] = ii;
    }
    __syncthreads();
    uint32_t m = 0;  // entries written so far (block-uniform)
    for (uint32_t base = 0; base < kp; base += PT) {
        const uint32_t i = base + tid;
        float c = 0.0f;
        bool keep = false;
        if (i < kp) {
            c = __uint_as_float(total_key_bits(skey[i]));
            keep = !a.has_min || c >= a.min_conf;
        }
        uint32_t tot;
        const uint32_t pos = m + block_scan(keep ? 1u : 0u, sw, tot);
        if (keep) {
            io[pos] = sidx[i];
            co[pos] = c;
        }
        m += tot;
    }
    // slots past the count are defined (zero), as in the step's own rows
    for (uint32_t j = m + tid; j < K; j += PT) {
        io[j] = 0u;
        co[j] = 0.0f;
    }
    if (tid == 0) a.count_out[row] = m;
}

struct AfterArgs {
    const uint32_t *in_idx;  // the step's packed rows: [rows, k]
    const float *in_conf;
    const uint32_t *in_cnt;  // [rows]
    const float *table;
    const int32_t *sites;
    uint32_t *idx_out;  // [rows, k_stride]
    float *conf_out;
    uint32_t *count_out;
    int64_t tstride, k_stride, n;
    uint32_t n_sites, k;
    int32_t site, rerank;
    float thr;
};

// dynamic LDS: key[k] | conf bits[k] | admitted[k]
__global__ __launch_bounds__(PT) void prior_after_kernel(AfterArgs a) {
    extern __shared__ __align__(16) uint32_t dyn[];
    __shared__ uint32_t sw[4];
    const uint32_t tid = threadIdx.x, K = a.k;
    const int64_t row = blockIdx.x;
    uint32_t s = a.sites ? (uint32_t)a.sites[row] : (uint32_t)a.site;
    if (s >= a.n_sites) s = 0;
    const float *pr = a.table + (int64_t)s * a.tstride;
    const uint32_t *ii = a.in_idx + row * (int64_t)K;
    const float *ic = a.in_conf + row * (int64_t)K;
    uint32_t *key = dyn, *cbits = dyn + K, *adm = dyn + 2 * (size_t)K;
    uint32_t *io = a.idx_out + row * a.k_stride;
    float *co = a.conf_out + row * a.k_stride;
    const uint32_t cnt = std::min(a.in_cnt[row], K);
    uint32_t mine = 0;
    for (uint32_t i = tid; i < cnt; i += PT) {
        const uint32_t sp = ii[i];
        const float p = (int64_t)sp < a.n ? pr[sp] : -1.0f;
        const float c = prior_conf(ic[i], p, a.rerank);
        const uint32_t ad = admitted(p, a.thr) ? 1u : 0u;
        cbits[i] = __float_as_uint(c);
        adm[i] = ad;
        key[i] = a.rerank ? total_key(__float_as_uint(c)) : 0u;  // without reranking the order is the input's
        mine += ad;
    }
    uint32_t m;
    (void)block_scan(mine, sw, m);  // its barriers also publish the arrays
    for (uint32_t i = tid; i < cnt; i += PT) {
        if (!adm[i]) continue;
        const uint32_t ki = key[i];
        uint32_t r = 0;
        for (uint32_t j = 0; j < cnt; j++) {
            const uint32_t kj = key[j];
            r += (adm[j] && (kj > ki || (kj == ki && j < i))) ? 1u : 0u;
        }
        io[r] = ii[i];
        co[r] = __uint_as_float(cbits[i]);
    }
    for (uint32_t j = m + tid; j < K; j += PT) {
        io[j] = 0u;
        co[j] = 0.0f;
    }
    if (tid == 0) a.count_out[row] = m;
}

size_t select_lds_bytes(int64_t n) { return (size_t)n * sizeof(uint32_t); }
size_t after_lds_bytes(size_t k) { return 3 * k * sizeof(uint32_t); }

}  // namespace

void register_prior_kernels() {
    register_dynamic_lds_kernel(reinterpret_cast<const void *>(prior_select_kernel<false>));
    register_dynamic_lds_kernel(reinterpret_cast<const void *>(prior_after_kernel));
}

}  // namespace bn

struct bn_prior {
    std::atomic<int> refs{1};  // the caller's handle + one per context that attached it
    int device = 0;
    size_t n_sites = 0, n_species = 0, tstride = 0;  // device rows are padded to a multiple of 4 floats: every row 16-byte aligned
    float threshold = 0.f;
    uint32_t flags = 0;
    bn::Stream stream;  // bn_prior_apply_host's, created on first use; before the table: it goes last (device_mem.h)
    bn::DeviceBuf<float> d_table;  // [n_sites, tstride]
    std::mutex mu;                 // bn_prior_apply_host / bn_prior_read: one thread at a time
    ~bn_prior() {
        (void)bn::use_device(device);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

struct bn::PriorAttach {
    bn_prior *prior = nullptr;
    size_t max_batch = 0, top_k = 0;
    int32_t has_min = 0;
    float min_conf = 0.f;
    bool has_map = false;
    std::vector<int32_t> source_sites;
    int32_t site = 0;
    bn::TopkRows rows;            // the last step's filtered rows: device block and pinned mirror
    bn::DeviceBuf<uint32_t> d_gkeys;  // general select form: [max_batch, n_species]
    bn::PinnedRing sites;  // per-row site ids of a live step under a map: [max_batch] int32, read by the kernel in place
    ~PriorAttach();        // drops the reference
};

namespace {

using bn::set_last_error;

using bn::check_launch;

constexpr uint32_t KNOWN_FLAGS = BN_PRIOR_AFTER_TOPK | BN_PRIOR_RERANK;

void prior_unref(bn_prior *p) {
    if (p && p->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) delete p;
}

bool general_form(const bn_prior *p) { return (int64_t)p->n_species > bn::SEL_LDS_MAX_N || bn::sw_present(bn::sw::BN_PRIOR_GENERAL); }

// the K of a select row, or 0 with the refusal's message set
size_t select_k(const bn_prior *p, size_t top_k) {
    if (top_k < 1 || top_k > bn::SEL_K_MAX) {
        (void)set_last_error(BN_ERR_INVALID_ARG, "a prior's top_k must be in 1..1024, got " + std::to_string(top_k));
        return 0;
    }
    return std::min(top_k, p->n_species);
}

// SELECT on `rows` device rows; sites: device-readable [rows] or NULL (every row at `site`)
bn_status enqueue_select(const bn_prior *p, hipStream_t stream, const float *d_logits, size_t rows, const int32_t *sites, int32_t site, size_t k,
                         int32_t has_min, float min_conf, size_t k_stride, uint32_t *d_gkeys, uint32_t *d_idx, float *d_conf, uint32_t *d_cnt) {
    bn::SelectArgs a{};
    a.logits = d_logits;
    a.table = p->d_table;
    a.sites = sites;
    a.gkeys = d_gkeys;
    a.idx_out = d_idx;
    a.conf_out = d_conf;
    a.count_out = d_cnt;
    a.n = (int64_t)p->n_species;
    a.tstride = (int64_t)p->tstride;
    a.k_stride = (int64_t)k_stride;
    a.n_sites = (uint32_t)p->n_sites;
    a.k = (uint32_t)k;
    a.site = site;
    a.rerank = (p->flags & BN_PRIOR_RERANK) ? 1 : 0;
    a.has_min = has_min ? 1 : 0;
    a.thr = p->threshold;
    a.min_conf = min_conf;
    (void)hipGetLastError();
    if (d_gkeys) {
        hipLaunchKernelGGL(bn::prior_select_kernel<true>, dim3((unsigned)rows), dim3(bn::PT), 0, stream, a);
    } else {
        const size_t lds = bn::select_lds_bytes(a.n);
        // static + dynamic LDS together pass the default limit from about 11 000 species on
        if (!bn::ensure_dynamic_lds(reinterpret_cast<const void *>(bn::prior_select_kernel<false>), lds + 24 * 1024))
            return set_last_error(BN_ERR_BACKEND, "the prior kernel needs more LDS than the device grants");
        hipLaunchKernelGGL(bn::prior_select_kernel<false>, dim3((unsigned)rows), dim3(bn::PT), lds, stream, a);
    }
    return check_launch("prior select");
}

bn_status enqueue_after(const bn_prior *p, hipStream_t stream, const uint32_t *in_idx, const float *in_conf, const uint32_t *in_cnt, size_t rows,
                        const int32_t *sites, int32_t site, size_t k, size_t k_stride, uint32_t *d_idx, float *d_conf, uint32_t *d_cnt) {
    bn::AfterArgs a{};
    a.in_idx = in_idx;
    a.in_conf = in_conf;
    a.in_cnt = in_cnt;
    a.table = p->d_table;
    a.sites = sites;
    a.idx_out = d_idx;
    a.conf_out = d_conf;
    a.count_out = d_cnt;
    a.tstride = (int64_t)p->tstride;
    a.k_stride = (int64_t)k_stride;
    a.n = (int64_t)p->n_species;
    a.n_sites = (uint32_t)p->n_sites;
    a.k = (uint32_t)k;
    a.site = site;
    a.rerank = (p->flags & BN_PRIOR_RERANK) ? 1 : 0;
    a.thr = p->threshold;
    const size_t lds = bn::after_lds_bytes(k);
    (void)hipGetLastError();
    if (!bn::ensure_dynamic_lds(reinterpret_cast<const void *>(bn::prior_after_kernel), lds))
        return set_last_error(BN_ERR_BACKEND, "the prior kernel needs more LDS than the device grants");
    hipLaunchKernelGGL(bn::prior_after_kernel, dim3((unsigned)rows), dim3(bn::PT), lds, stream, a);
    return check_launch("prior filter");
}

bn_status check_site(const bn_prior *p, int64_t site, const char *what) {
    if (site < 0 || (uint64_t)site >= p->n_sites)
        return set_last_error(BN_ERR_INVALID_ARG, std::string(what) + " " + std::to_string(site) + " is outside 0.." + std::to_string(p->n_sites));
    return BN_OK;
}

}  // namespace

bn_status bn::prior_attach(bn_prior *p, int device, size_t num_species, size_t max_batch, const int32_t *source_sites, size_t n_source_sites, size_t top_k,
                           int32_t has_min, float min_conf, PriorAttach **out) {
    if (!p || !out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (num_species != p->n_species)
        return set_last_error(BN_ERR_INVALID_ARG, "the prior has " + std::to_string(p->n_species) + " species, the model " + std::to_string(num_species));
    if (device != p->device)
        return set_last_error(BN_ERR_INVALID_ARG, "the context lives on device " + std::to_string(device) + ", the prior on " + std::to_string(p->device));
    if (n_source_sites && !source_sites) return set_last_error(BN_ERR_INVALID_ARG, "null source_sites with a non-zero count");
    const bool after = (p->flags & BN_PRIOR_AFTER_TOPK) != 0;
    size_t k = 0;
    if (!after && (k = select_k(p, top_k)) == 0) return BN_ERR_INVALID_ARG;
    for (size_t i = 0; i < n_source_sites; i++) {
        bn_status st = check_site(p, source_sites[i], "the site of a source,");
        if (st != BN_OK) return st;
    }
    BN_HIP_TRY(bn::use_device(device));
    auto a = std::make_unique<PriorAttach>();
    a->max_batch = max_batch;
    a->top_k = top_k;
    a->has_min = has_min;
    a->min_conf = min_conf;
    a->has_map = source_sites != nullptr;
    if (source_sites) a->source_sites.assign(source_sites, source_sites + n_source_sites);
    if (!after) {
        bn_status st = a->rows.reserve(max_batch, k, nullptr, true, true);
        if (st != BN_OK) return st;
        if (general_form(p)) BN_HIP_TRY(a->d_gkeys.alloc(max_batch * p->n_species * sizeof(uint32_t)));
    }
    BN_HIP_TRY(a->sites.create(std::max<size_t>(max_batch, 1) * sizeof(int32_t)));
    p->refs.fetch_add(1, std::memory_order_relaxed);
    a->prior = p;
    *out = a.release();
    return BN_OK;
}

bn::PriorAttach::~PriorAttach() { prior_unref(prior); }
void bn::prior_detach(PriorAttach *a) { delete a; }

bn_status bn::prior_set_site(PriorAttach *a, int32_t site) {
    bn_status st = check_site(a->prior, site, "site");
    if (st != BN_OK) return st;
    a->site = site;
    return BN_OK;
}

bn_status bn::prior_step_check(const PriorAttach *a, size_t n_sources) {
    if (a->has_map && n_sources > a->source_sites.size())
        return set_last_error(BN_ERR_INVALID_ARG, "the pool has " + std::to_string(n_sources) + " sources, the attached prior's site map " +
                                                      std::to_string(a->source_sites.size()));
    return BN_OK;
}

bn_status bn::prior_step(PriorAttach *a, hipStream_t stream, const float *d_logits, const TopkRows::ConstView &step_rows, const StepRows &rows) {
    const bn_prior *p = a->prior;
    const size_t batch = rows.batch;
    if (batch > a->max_batch) return set_last_error(BN_ERR_INVALID_ARG, "batch exceeds the context's max_batch");
    const bool after = (p->flags & BN_PRIOR_AFTER_TOPK) != 0;
    const size_t k = after ? step_rows.k : std::min(a->top_k, p->n_species);
    bn_status st = a->rows.reserve(a->max_batch, k, stream, true, true);
    if (st != BN_OK) return st;
    // the rows' sites by their sources, in pinned memory the kernel reads in place: no copy, no synchronisation
    const int32_t *sites = nullptr;
    int slot = -1;
    if (a->has_map && rows.sources) {
        void *hp = nullptr;
        BN_HIP_TRY(a->sites.acquire(&slot, &hp));
        for (size_t i = 0; i < batch; i++) {
            const int32_t src = rows.sources[i];
            if (src < 0 || (size_t)src >= a->source_sites.size()) return set_last_error(BN_ERR_INVALID_ARG, "a source outside the attached prior's site map");
            static_cast<int32_t *>(hp)[i] = a->source_sites[(size_t)src];
        }
        sites = static_cast<const int32_t *>(a->sites.device_ptr(slot));
    }
    const TopkRows::View out = TopkRows::view(a->rows.d, batch, k);
    if (after)
        st = enqueue_after(p, stream, step_rows.idx, step_rows.conf, step_rows.count, batch, sites, a->site, k, k, out.idx, out.conf, out.count);
    else
        st = enqueue_select(p, stream, d_logits, batch, sites, a->site, k, a->has_min, a->min_conf, k, a->d_gkeys, out.idx, out.conf, out.count);
    if (st != BN_OK) return st;
    if (sites) BN_HIP_TRY(a->sites.commit(slot, stream));
    const bn::OutRegion reg{a->rows.h, a->rows.d, TopkRows::bytes(batch, k)};
    if ((st = bn::results_to_host(stream, &reg, 1)) != BN_OK) return st;
    a->rows.mark(batch, k);
    return BN_OK;
}

bn::PriorView bn::prior_view(const bn_prior *p) {
    return PriorView{p->device, p->d_table, p->n_sites, p->n_species, p->tstride, p->threshold, (p->flags & BN_PRIOR_RERANK) ? 1 : 0};
}

const bn_prior *bn::prior_of(const PriorAttach *a) { return a ? a->prior : nullptr; }

int32_t bn::prior_site_of(const PriorAttach *a, int32_t source) {
    if (a->has_map && source >= 0 && (size_t)source < a->source_sites.size()) return a->source_sites[(size_t)source];
    return a->site;
}

bn_status bn::prior_step_results(const PriorAttach *a, const uint32_t **idx, const float **conf, const uint32_t **count, size_t *k_stride) {
    static const char *none = "no step has run on this context since a prior was attached";
    if (!a) return set_last_error(BN_ERR_INVALID_ARG, none);
    return a->rows.results(none, idx, conf, count, k_stride);
}

extern "C" {

bn_status bn_prior_create(int32_t device, size_t n_sites, size_t n_species, const float *table, float threshold, uint32_t flags, bn_prior **out) {
    if (!out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!table) return set_last_error(BN_ERR_INVALID_ARG, "null table");
    if (n_sites == 0 || n_species == 0) return set_last_error(BN_ERR_INVALID_ARG, "a prior needs at least one site and one species");
    if (n_sites > 0x7fffffffu || n_species > 0x7fffffffu) return set_last_error(BN_ERR_INVALID_ARG, "n_sites and n_species must be below 2^31");
    if (flags & ~KNOWN_FLAGS) return set_last_error(BN_ERR_INVALID_ARG, "unknown flag bits " + std::to_string(flags & ~KNOWN_FLAGS));
    if (!std::isfinite(threshold)) return set_last_error(BN_ERR_INVALID_ARG, "the threshold must be finite");
    for (size_t i = 0; i < n_sites * n_species; i++)
        if (!std::isfinite(table[i]))
            return set_last_error(BN_ERR_INVALID_ARG, "table entry [" + std::to_string(i / n_species) + "][" + std::to_string(i % n_species) + "] is not finite");
    if (bn_status dst = bn::require_device(device); dst != BN_OK) return dst;
    BN_HIP_TRY(bn::use_device(device));
    if (!bn::prepare_device(device)) return set_last_error(BN_ERR_BACKEND, "device refused the kernels' dynamic-LDS opt-in");
    auto p = std::make_unique<bn_prior>();
    p->device = device;
    p->n_sites = n_sites;
    p->n_species = n_species;
    p->tstride = (n_species + 3) / 4 * 4;
    p->threshold = threshold;
    p->flags = flags;
    BN_HIP_TRY(p->d_table.alloc(n_sites * p->tstride * sizeof(float)));
    if (p->tstride == n_species) {
        BN_HIP_TRY(bn::gated::Memcpy(p->d_table, table, n_sites * n_species * sizeof(float), hipMemcpyHostToDevice));
    } else {
        std::vector<float> pad(n_sites * p->tstride, BN_PRIOR_UNKNOWN);
        for (size_t s = 0; s < n_sites; s++) memcpy(pad.data() + s * p->tstride, table + s * n_species, n_species * sizeof(float));
        BN_HIP_TRY(bn::gated::Memcpy(p->d_table, pad.data(), pad.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    *out = p.release();
    return BN_OK;
}

void bn_prior_free(bn_prior *p) { prior_unref(p); }

size_t bn_prior_sites(const bn_prior *p) { return p ? p->n_sites : 0; }
size_t bn_prior_species(const bn_prior *p) { return p ? p->n_species : 0; }
float bn_prior_threshold(const bn_prior *p) { return p ? p->threshold : 0.f; }
uint32_t bn_prior_flags(const bn_prior *p) { return p ? p->flags : 0; }

bn_status bn_prior_read(const bn_prior *pc, size_t first_site, size_t count, float *out) {
    if (!pc) return set_last_error(BN_ERR_INVALID_ARG, "null prior");
    if (first_site > pc->n_sites || count > pc->n_sites - first_site) return set_last_error(BN_ERR_INVALID_ARG, "sites outside the table");
    if (count == 0) return BN_OK;
    if (!out) return set_last_error(BN_ERR_INVALID_ARG, "null output");
    bn_prior *p = const_cast<bn_prior *>(pc);
    std::lock_guard<std::mutex> lk(p->mu);
    BN_HIP_TRY(bn::use_device(p->device));
    bn::gated::Shared gate;
    BN_HIP_TRY(hipMemcpy2D(out, p->n_species * sizeof(float), p->d_table + first_site * p->tstride, p->tstride * sizeof(float),
                          p->n_species * sizeof(float), count, hipMemcpyDeviceToHost));
    return BN_OK;
}

bn_status bn_prior_apply_host(const bn_prior *pc, const float *logits, size_t rows, const int32_t *sites, size_t top_k, int32_t has_min, float min_conf,
                              size_t k_stride, uint32_t *idx_out, float *conf_out, uint32_t *count_out) {
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!pc) return set_last_error(BN_ERR_INVALID_ARG, "null prior");
    if (rows == 0) return BN_OK;
    if (!logits || !sites || !idx_out || !conf_out || !count_out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    bn_prior *p = const_cast<bn_prior *>(pc);  // the stream is not part of the prior's value
    const bool after = (p->flags & BN_PRIOR_AFTER_TOPK) != 0;
    const size_t n = p->n_species;
    size_t k = 0;
    if (after) {
        bn_status kst = bn::check_top_k(n, top_k, &k);
        if (kst != BN_OK) return kst;
    } else if ((k = select_k(p, top_k)) == 0) {
        return BN_ERR_INVALID_ARG;
    }
    if (k_stride < k) return set_last_error(BN_ERR_INVALID_ARG, "k_stride " + std::to_string(k_stride) + " is below min(top_k, n_species) = " + std::to_string(k));
    for (size_t r = 0; r < rows; r++) {
        bn_status st = check_site(p, sites[r], "the site of a row,");
        if (st != BN_OK) return st;
    }
    std::lock_guard<std::mutex> lk(p->mu);
    BN_HIP_TRY(bn::use_device(p->device));
    if (!p->stream) BN_HIP_TRY(p->stream.create(hipStreamNonBlocking));
    bn::Scratch bufs;
    bufs.stream = p->stream;  // the prior's own: waited for, not destroyed
    constexpr size_t CHUNK = 1024;  // rows per round
    const size_t cr = std::min(CHUNK, rows);
    float *d_logits = nullptr, *d_conf = nullptr;
    int32_t *d_sites = nullptr;
    uint32_t *d_idx = nullptr, *d_cnt = nullptr, *d_gkeys = nullptr, *d_tk = nullptr, *d_flags = nullptr;
    BN_HIP_TRY(bufs.alloc(&d_logits, cr * n * sizeof(float)));
    BN_HIP_TRY(bufs.alloc(&d_sites, cr * sizeof(int32_t)));
    BN_HIP_TRY(bufs.alloc(&d_idx, cr * k * sizeof(uint32_t)));
    BN_HIP_TRY(bufs.alloc(&d_conf, cr * k * sizeof(float)));
    BN_HIP_TRY(bufs.alloc(&d_cnt, cr * sizeof(uint32_t)));
    if (after) {
        BN_HIP_TRY(bufs.alloc(&d_tk, bn::TopkRows::bytes(cr, k)));  // the rows of a chunk's own top-K
        BN_HIP_TRY(bufs.alloc(&d_flags, cr * sizeof(uint32_t)));
    } else if (general_form(p)) {
        BN_HIP_TRY(bufs.alloc(&d_gkeys, cr * n * sizeof(uint32_t)));
    }
    std::vector<uint32_t> h_idx(cr * k), h_cnt(cr);
    std::vector<float> h_conf(cr * k);
    for (size_t r0 = 0; r0 < rows; r0 += CHUNK) {
        const size_t m = std::min(CHUNK, rows - r0);
        BN_HIP_TRY(bn::gated::Memcpy(d_logits, logits + r0 * n, m * n * sizeof(float), hipMemcpyHostToDevice));
        BN_HIP_TRY(bn::gated::Memcpy(d_sites, sites + r0, m * sizeof(int32_t), hipMemcpyHostToDevice));
        bn_status st;
        if (after) {
            const bn::TopkRows::View t = bn::TopkRows::view(d_tk, m, k);
            if ((st = bn::enqueue_topk_rows(p->stream, d_logits, m, n, k, has_min, min_conf, t, d_flags)) != BN_OK) return st;
            st = enqueue_after(p, p->stream, t.idx, t.conf, t.count, m, d_sites, 0, k, k, d_idx, d_conf, d_cnt);
        } else {
            st = enqueue_select(p, p->stream, d_logits, m, d_sites, 0, k, has_min, min_conf, k, d_gkeys, d_idx, d_conf, d_cnt);
        }
        if (st != BN_OK) return st;
        BN_HIP_TRY(hipStreamSynchronize(p->stream));
        BN_HIP_TRY(bn::gated::Memcpy(h_idx.data(), d_idx, m * k * sizeof(uint32_t), hipMemcpyDeviceToHost));
        BN_HIP_TRY(bn::gated::Memcpy(h_conf.data(), d_conf, m * k * sizeof(float), hipMemcpyDeviceToHost));
        BN_HIP_TRY(bn::gated::Memcpy(h_cnt.data(), d_cnt, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t r = 0; r < m; r++) {
            memcpy(idx_out + (r0 + r) * k_stride, h_idx.data() + r * k, k * sizeof(uint32_t));
            memcpy(conf_out + (r0 + r) * k_stride, h_conf.data() + r * k, k * sizeof(float));
            count_out[r0 + r] = h_cnt[r];
        }
    }
    return BN_OK;
}

}  // extern "C"
