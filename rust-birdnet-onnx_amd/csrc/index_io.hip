// Persistence of an embedding index behind the C ABI (include/birdnet_hip.h, bn_index_save / bn_index_load): the slab's stored bits to
// a file and back.  The format, its header and the host-only entry points are in index_file.h / index_file.cpp; the digest is
// index_digest.h, shared with them.
//
// Kernels (one wave per row; a launch covers a SLICE: the rows that fit one staging block, whatever the chunk size -- a chunk's digest
// is a sum, so slices and chunks need not line up):
//   * index_pack_kernel    -- reads padded slab rows [n, dpad], writes them with stride dim into a device staging block, and adds
//     digest_term of every element to the row's chunk slot; counts the rows whose valid byte is set.
//   * index_restore_kernel -- the mirror: staging rows [n, dim] into the padded slab with the pad columns zeroed, the valid byte of
//     each row from the all-zero rule, the same digest, the count of valid rows, and the first chunk that holds a non-finite element
//     (integer atomicMin).
// Both accumulate per-thread 64-bit sums, reduce them over the wave, and add once per block to the chunk's slot (a block whose four
// rows straddle a chunk boundary adds once per chunk): integer atomics only, so every order gives the same bytes.
// Access width: with dim % 4 == 0 every row of both layouts starts on a 16-byte boundary (dpad is a multiple of 128, the staging
// block is allocated) and a lane moves 16 bytes; otherwise the two layouts' 16-byte phases differ from row to row, one side of any
// wide access would be misaligned, and the lanes move consecutive dwords (still one contiguous 256-byte run per wave instruction).
//
// Pipelines: two device staging blocks and two pinned blocks of STAGE_BYTES.  Save: pack slice i, copy it to pinned block i % 2, and
// while the host thread writes that block to the file slices i + 1 is packed and copied.  Load: the host thread read()s slice i + 1
// into the other pinned block while slice i is copied up and restored.  Digests, the valid count and the non-finite flag are compared
// on the host once, at the end; only then does the index take its size (index_adopt_rows) or the file its name (rename).
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "hip_gate.h"
#include "index_digest.h"
#include "index_file.h"

namespace {

constexpr size_t STAGE_BYTES = 8u << 20;  // >= one row: dim <= 2^20
constexpr int NBUF = 2;
constexpr uint32_t NO_CHUNK = 0xffffffffu;

using bn::check_launch;
using bn::digest_term;
using bn::set_last_error;
using u64 = unsigned long long;

__device__ inline uint64_t wave_sum(uint64_t v) {
    for (int off = 32; off; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, off), hi = __shfl_xor((uint32_t)(v >> 32), off);
        v += (uint64_t)hi << 32 | lo;
    }
    return v;
}

// the four waves' (chunk, digest sum, valid rows) -> one add per chunk the block's rows touch (their chunks do not decrease)
__device__ inline void block_commit(uint32_t chunk, uint64_t sum, uint32_t nvalid, uint32_t rows_here, u64 *__restrict__ digest, u64 *__restrict__ valid_rows) {
    __shared__ uint64_t s_sum[4];
    __shared__ uint32_t s_chunk[4], s_valid[4];
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_sum[w] = sum;
        s_chunk[w] = chunk;
        s_valid[w] = nvalid;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t cur = s_chunk[0], nv = s_valid[0];
    uint64_t acc = s_sum[0];
    for (uint32_t i = 1; i < rows_here; i++) {
        nv += s_valid[i];
        if (s_chunk[i] == cur) {
            acc += s_sum[i];
        } else {
            atomicAdd(digest + cur, (u64)acc);
            cur = s_chunk[i];
            acc = s_sum[i];
        }
    }
    atomicAdd(digest + cur, (u64)acc);
    if (nv) atomicAdd(valid_rows, (u64)nv);
}

// slab rows [row0, row0 + n) -> stage [n, dim]; grid = ceil(n / 4) blocks of 4 waves
template <bool V4>
__global__ __launch_bounds__(256) void index_pack_kernel(const uint32_t *__restrict__ slab, const uint8_t *__restrict__ valid, uint32_t row0, uint32_t n,
                                                         uint32_t dim, uint32_t dpad, uint32_t chunk_rows, uint32_t *__restrict__ stage,
                                                         u64 *__restrict__ digest, u64 *__restrict__ valid_rows) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
    uint64_t sum = 0;
    uint32_t chunk = 0, nvalid = 0;
    if (r < n) {
        const uint32_t id = row0 + r;
        chunk = id / chunk_rows;
        const uint32_t *x = slab + (size_t)id * dpad;
        uint32_t *y = stage + (size_t)r * dim;
        const uint64_t u0 = (uint64_t)id * dim;
        if (V4) {
            for (uint32_t k = 4 * lane; k < dim; k += 256) {
                const uint4 v = *reinterpret_cast<const uint4 *>(x + k);
                *reinterpret_cast<uint4 *>(y + k) = v;
                sum += digest_term(u0 + k, v.x) + digest_term(u0 + k + 1, v.y) + digest_term(u0 + k + 2, v.z) + digest_term(u0 + k + 3, v.w);
            }
        } else {
            for (uint32_t k = lane; k < dim; k += 64) {
                const uint32_t b = x[k];
                y[k] = b;
                sum += digest_term(u0 + k, b);
            }
        }
        nvalid = valid[id] ? 1 : 0;
    }
    sum = wave_sum(sum);
    block_commit(chunk, sum, nvalid, min(4u, n - blockIdx.x * 4), digest, valid_rows);
}

// stage [n, dim] -> slab rows [row0, row0 + n), pad columns zeroed, valid bytes written; *bad_chunk: the first chunk with a non-finite element
template <bool V4>
__global__ __launch_bounds__(256) void index_restore_kernel(const uint32_t *__restrict__ stage, uint32_t row0, uint32_t n, uint32_t dim, uint32_t dpad,
                                                            uint32_t chunk_rows, uint32_t *__restrict__ slab, uint8_t *__restrict__ valid,
                                                            u64 *__restrict__ digest, u64 *__restrict__ valid_rows, uint32_t *__restrict__ bad_chunk) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
    uint64_t sum = 0;
    uint32_t chunk = 0, nvalid = 0;
    if (r < n) {
        const uint32_t id = row0 + r;
        chunk = id / chunk_rows;
        const uint32_t *x = stage + (size_t)r * dim;
        uint32_t *y = slab + (size_t)id * dpad;
        const uint64_t u0 = (uint64_t)id * dim;
        bool nonzero = false, finite = true;
        if (V4) {
            for (uint32_t k = 4 * lane; k < dim; k += 256) {
                const uint4 v = *reinterpret_cast<const uint4 *>(x + k);
                *reinterpret_cast<uint4 *>(y + k) = v;
                sum += digest_term(u0 + k, v.x) + digest_term(u0 + k + 1, v.y) + digest_term(u0 + k + 2, v.z) + digest_term(u0 + k + 3, v.w);
                nonzero = nonzero || !(bn::digest_is_zero(v.x) && bn::digest_is_zero(v.y) && bn::digest_is_zero(v.z) && bn::digest_is_zero(v.w));
                finite = finite && bn::digest_is_finite(v.x) && bn::digest_is_finite(v.y) && bn::digest_is_finite(v.z) && bn::digest_is_finite(v.w);
            }
            for (uint32_t k = dim + 4 * lane; k < dpad; k += 256) *reinterpret_cast<uint4 *>(y + k) = make_uint4(0u, 0u, 0u, 0u);
        } else {
            for (uint32_t k = lane; k < dim; k += 64) {
                const uint32_t b = x[k];
                y[k] = b;
                sum += digest_term(u0 + k, b);
                nonzero = nonzero || !bn::digest_is_zero(b);
                finite = finite && bn::digest_is_finite(b);
            }
            for (uint32_t k = dim + lane; k < dpad; k += 64) y[k] = 0u;
        }
        const bool row_valid = __ballot(nonzero) != 0;
        const bool row_finite = __ballot(!finite) == 0;
        if (lane == 0) {
            valid[id] = row_valid ? 1 : 0;
            if (!row_finite) atomicMin(bad_chunk, chunk);
        }
        nvalid = row_valid ? 1 : 0;
    }
    sum = wave_sum(sum);
    block_commit(chunk, sum, nvalid, min(4u, n - blockIdx.x * 4), digest, valid_rows);
}

// The buffers of one save or load on the index's stream: on every way out the stream is waited for before anything is freed.
// d_meta: [n_chunks] chunk digests, then the valid-row count, then (low word) the first chunk with a non-finite element
struct IoBuffers {
    hipStream_t stream = nullptr;
    bn::DeviceBuf<uint32_t> d_stage[NBUF];
    bn::PinnedBuf<uint32_t> h_stage[NBUF];
    bn::Event ev[NBUF];
    bn::DeviceBuf<u64> d_meta;
    bn_status create(hipStream_t s, size_t n_chunks) {
        stream = s;
        for (int b = 0; b < NBUF; b++) {
            BN_HIP_TRY(d_stage[b].alloc(STAGE_BYTES));
            BN_HIP_TRY(h_stage[b].alloc(STAGE_BYTES));
            BN_HIP_TRY(ev[b].create(hipEventDisableTiming));
        }
        BN_HIP_TRY(d_meta.alloc((n_chunks + 2) * sizeof(u64)));
        BN_HIP_TRY(hipMemsetAsync(d_meta, 0, (n_chunks + 1) * sizeof(u64), stream));
        BN_HIP_TRY(hipMemsetAsync(d_meta + n_chunks + 1, 0xff, sizeof(u64), stream));
        return BN_OK;
    }
    ~IoBuffers() {
        if (stream) (void)hipStreamSynchronize(stream);
    }
    // the stream's work done; digests [n_chunks], the valid-row count and the non-finite chunk to the host
    bn_status read_meta(size_t n_chunks, std::vector<uint64_t> *meta) {
        meta->resize(n_chunks + 2);
        BN_HIP_TRY(hipStreamSynchronize(stream));
        BN_HIP_TRY(bn::gated::Memcpy(meta->data(), d_meta, (n_chunks + 2) * sizeof(u64), hipMemcpyDeviceToHost));
        return BN_OK;
    }
};

std::atomic<uint64_t> g_temp_counter{0};

size_t slice_rows(size_t dim) { return std::max<size_t>(1, STAGE_BYTES / (dim * sizeof(float))); }

using bn::index_file::Fd;

// the temporary of a save: removed unless the rename happened
struct TempFile {
    std::string name;
    bool keep = false;
    ~TempFile() {
        if (!name.empty() && !keep) (void)::unlink(name.c_str());
    }
};

bool write_at(int fd, const void *src, size_t n, uint64_t off) {
    const uint8_t *p = static_cast<const uint8_t *>(src);
    while (n) {
        const ssize_t put = ::pwrite(fd, p, n, (off_t)off);
        if (put < 0 && errno == EINTR) continue;
        if (put <= 0) return false;
        p += put;
        off += (uint64_t)put;
        n -= (size_t)put;
    }
    return true;
}

bn_status save(bn_index *x, const char *path, size_t chunk_rows_arg) {
    namespace f = bn::index_file;
    if (!x) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    if (!path || !*path) return set_last_error(BN_ERR_INVALID_ARG, "null path");
    if (chunk_rows_arg > 0xffffffffull) return set_last_error(BN_ERR_INVALID_ARG, "chunk_rows above 2^32 - 1");
    bn::IndexIo io;
    bn_status st = bn::index_io_state(x, &io);
    if (st != BN_OK) return st;
    f::Header h;
    h.dim = (uint32_t)io.dim;
    h.rows = io.size;
    h.chunk_rows = (uint32_t)(chunk_rows_arg ? chunk_rows_arg : f::default_chunk_rows(io.dim));
    h.n_chunks = f::chunk_count(h.rows, h.chunk_rows);

    // "<path>.tmp.<pid>.<n>", n from a counter of the process: two threads saving to one path get two names, and a name a crashed
    // process with this pid left behind is stepped over (O_EXCL never opens a file that exists)
    TempFile tmp;
    Fd out;
    std::string temp_name;
    for (int attempt = 0; attempt < 64 && out.fd < 0; attempt++) {
        temp_name = std::string(path) + ".tmp." + std::to_string((long long)::getpid()) + "." + std::to_string(g_temp_counter.fetch_add(1));
        out.fd = ::open(temp_name.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0644);
        if (out.fd < 0 && errno != EEXIST) break;
    }
    if (out.fd < 0) return set_last_error(BN_ERR_INVALID_ARG, "cannot create " + temp_name + ": " + strerror(errno));
    tmp.name = temp_name;
    const auto io_error = [&](const char *what) { return set_last_error(BN_ERR_BACKEND, std::string(what) + " " + temp_name + " failed: " + strerror(errno)); };

    IoBuffers buf;
    if ((st = buf.create(io.stream, h.n_chunks)) != BN_OK) return st;
    const size_t sr = slice_rows(io.dim);
    const size_t n_slices = (h.rows + sr - 1) / sr;
    const bool v4 = io.dim % 4 == 0;
    const auto issue = [&](size_t i) -> bn_status {
        const int b = (int)(i % NBUF);
        const size_t r0 = i * sr, n = std::min(sr, (size_t)h.rows - r0);
        const dim3 grid((unsigned)((n + 3) / 4)), block(256);
        const uint32_t *slab = reinterpret_cast<const uint32_t *>(io.slab);
        if (v4)
            hipLaunchKernelGGL(index_pack_kernel<true>, grid, block, 0, io.stream, slab, io.valid, (uint32_t)r0, (uint32_t)n, h.dim, (uint32_t)io.dpad,
                               h.chunk_rows, buf.d_stage[b], buf.d_meta, buf.d_meta + h.n_chunks);
        else
            hipLaunchKernelGGL(index_pack_kernel<false>, grid, block, 0, io.stream, slab, io.valid, (uint32_t)r0, (uint32_t)n, h.dim, (uint32_t)io.dpad,
                               h.chunk_rows, buf.d_stage[b], buf.d_meta, buf.d_meta + h.n_chunks);
        if (bn_status ls = check_launch("index pack"); ls != BN_OK) return ls;
        BN_HIP_TRY(hipMemcpyAsync(buf.h_stage[b], buf.d_stage[b], n * io.dim * sizeof(float), hipMemcpyDeviceToHost, io.stream));
        BN_HIP_TRY(hipEventRecord(buf.ev[b], io.stream));
        return BN_OK;
    };
    for (size_t i = 0; i < std::min<size_t>(NBUF, n_slices); i++)
        if ((st = issue(i)) != BN_OK) return st;
    uint64_t off = f::payload_offset(h);
    for (size_t i = 0; i < n_slices; i++) {
        const int b = (int)(i % NBUF);
        const size_t bytes = std::min(sr, (size_t)h.rows - i * sr) * io.dim * sizeof(float);
        BN_HIP_TRY(hipEventSynchronize(buf.ev[b]));
        if (!write_at(out.fd, buf.h_stage[b], bytes, off)) return io_error("writing");
        off += bytes;
        // block b is free again: its slice is in the file, and the copy that filled it was the last reader of the device block
        if (i + NBUF < n_slices && (st = issue(i + NBUF)) != BN_OK) return st;
    }
    std::vector<uint64_t> meta;
    if ((st = buf.read_meta(h.n_chunks, &meta)) != BN_OK) return st;
    h.valid_rows = meta[h.n_chunks];
    uint8_t raw[f::HEADER_BYTES];
    f::encode_header(h, raw);
    if (h.n_chunks && !write_at(out.fd, meta.data(), (size_t)h.n_chunks * sizeof(uint64_t), f::table_offset())) return io_error("writing");
    if (!write_at(out.fd, raw, sizeof(raw), 0)) return io_error("writing");
    if (::fsync(out.fd) != 0) return io_error("flushing");
    if (out.reset() != 0) return io_error("closing");
    if (::rename(temp_name.c_str(), path) != 0) return io_error("renaming");
    tmp.keep = true;
    // the name as well as the bytes: flush the directory, where the file system lets a directory be opened and flushed
    const std::string full(path);
    const size_t slash = full.rfind('/');
    Fd dir;
    dir.fd = ::open(slash == std::string::npos ? "." : slash == 0 ? "/" : full.substr(0, slash).c_str(), O_RDONLY | O_DIRECTORY | O_CLOEXEC);
    if (dir.fd >= 0) (void)::fsync(dir.fd);
    return BN_OK;
}

bn_status load(int32_t device, const char *path, size_t capacity_rows, bn_index **out) {
    namespace f = bn::index_file;
    if (!out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!path) return set_last_error(BN_ERR_INVALID_ARG, "null path");
    f::Header h;
    Fd in;
    bn_status st = f::open_checked(path, &h, &in);
    if (st != BN_OK) return st;
    const size_t cap = capacity_rows ? capacity_rows : std::max<size_t>(1, (size_t)h.rows);
    if (cap < h.rows)
        return set_last_error(BN_ERR_INVALID_ARG, "capacity_rows " + std::to_string(cap) + " is below the file's " + std::to_string(h.rows) + " rows");
    if ((st = bn::require_device(device)) != BN_OK) return st;
    const std::string name(path);
    std::vector<uint64_t> table(h.n_chunks);
    if (h.n_chunks && !f::read_all(in.fd, table.data(), table.size() * sizeof(uint64_t))) return set_last_error(BN_ERR_MODEL_LOAD, name + ": read failed in the digest table");

    bn_index *raw = nullptr;
    if ((st = bn_index_create(device, h.dim, cap, &raw)) != BN_OK) return st;
    std::unique_ptr<bn_index, void (*)(bn_index *)> x(raw, bn_index_free);
    bn::IndexIo io;
    if ((st = bn::index_io_state(x.get(), &io)) != BN_OK) return st;
    IoBuffers buf;  // destroyed (stream waited for) before the index
    if ((st = buf.create(io.stream, h.n_chunks)) != BN_OK) return st;
    const size_t sr = slice_rows(io.dim);
    const size_t n_slices = (h.rows + sr - 1) / sr;
    const bool v4 = io.dim % 4 == 0;
    uint32_t *bad_chunk = reinterpret_cast<uint32_t *>(buf.d_meta + h.n_chunks + 1);
    for (size_t i = 0; i < n_slices; i++) {
        const int b = (int)(i % NBUF);
        const size_t r0 = i * sr, n = std::min(sr, (size_t)h.rows - r0);
        if (i >= NBUF) BN_HIP_TRY(hipEventSynchronize(buf.ev[b]));  // slice i - NBUF has left both blocks
        if (!f::read_all(in.fd, buf.h_stage[b], n * io.dim * sizeof(float))) return set_last_error(BN_ERR_MODEL_LOAD, name + ": read failed in the payload");
        BN_HIP_TRY(hipMemcpyAsync(buf.d_stage[b], buf.h_stage[b], n * io.dim * sizeof(float), hipMemcpyHostToDevice, io.stream));
        const dim3 grid((unsigned)((n + 3) / 4)), block(256);
        uint32_t *slab = reinterpret_cast<uint32_t *>(io.slab);
        if (v4)
            hipLaunchKernelGGL(index_restore_kernel<true>, grid, block, 0, io.stream, buf.d_stage[b], (uint32_t)r0, (uint32_t)n, h.dim, (uint32_t)io.dpad,
                               h.chunk_rows, slab, io.valid, buf.d_meta, buf.d_meta + h.n_chunks, bad_chunk);
        else
            hipLaunchKernelGGL(index_restore_kernel<false>, grid, block, 0, io.stream, buf.d_stage[b], (uint32_t)r0, (uint32_t)n, h.dim, (uint32_t)io.dpad,
                               h.chunk_rows, slab, io.valid, buf.d_meta, buf.d_meta + h.n_chunks, bad_chunk);
        if ((st = check_launch("index restore")) != BN_OK) return st;
        BN_HIP_TRY(hipEventRecord(buf.ev[b], io.stream));
    }
    std::vector<uint64_t> meta;
    if ((st = buf.read_meta(h.n_chunks, &meta)) != BN_OK) return st;
    for (size_t c = 0; c < h.n_chunks; c++)
        if (meta[c] != table[c])
            return set_last_error(BN_ERR_MODEL_LOAD, name + ": digest mismatch in chunk " + std::to_string(c) + " of " + std::to_string(h.n_chunks));
    const uint32_t bad = (uint32_t)meta[h.n_chunks + 1];
    if (bad != NO_CHUNK) return set_last_error(BN_ERR_MODEL_LOAD, name + ": non-finite element in chunk " + std::to_string(bad));
    if (meta[h.n_chunks] != h.valid_rows)
        return set_last_error(BN_ERR_MODEL_LOAD, name + ": the header counts " + std::to_string(h.valid_rows) + " valid rows, the payload holds " + std::to_string(meta[h.n_chunks]));
    if ((st = bn::index_adopt_rows(x.get(), (size_t)h.rows)) != BN_OK) return st;
    *out = x.release();
    return BN_OK;
}

}  // namespace

extern "C" {

bn_status bn_index_save(bn_index *x, const char *path, size_t chunk_rows) {
    try {
        return save(x, path, chunk_rows);
    } catch (const std::bad_alloc &) {
        return set_last_error(BN_ERR_BACKEND, "bn_index_save: out of host memory");
    }
}

bn_status bn_index_load(int32_t device, const char *path, size_t capacity_rows, bn_index **out) {
    try {
        return load(device, path, capacity_rows, out);
    } catch (const std::bad_alloc &) {
        return set_last_error(BN_ERR_BACKEND, "bn_index_load: out of host memory");
    }
}

}  // extern "C"
