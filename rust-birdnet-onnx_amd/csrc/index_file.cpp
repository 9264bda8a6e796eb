// Host side of the index file format (include/birdnet_hip.h, bn_index_save): the header, the size rule, and the two entry points that
// need no device -- bn_index_file_info and bn_index_file_verify.  The verifier recomputes every digest on the CPU from the one
// definition in index_digest.h; it shares no code with the kernels of index_io.hip beyond that function, which is what makes it
// the check of the device digests.  No HIP include (index_file.h).
#include "index_file.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <vector>

#include "index_digest.h"

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the digest table and the payload are written as the host holds them: little-endian");

namespace bn {
namespace index_file {
namespace {

const char MAGIC[8] = {'B', 'N', 'I', 'N', 'D', 'E', 'X', '1'};

void put32(uint8_t *p, uint32_t v) {
    for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i));
}
void put64(uint8_t *p, uint64_t v) {
    for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i));
}
uint32_t get32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
uint64_t get64(const uint8_t *p) { return (uint64_t)get32(p) | (uint64_t)get32(p + 4) << 32; }

// the sum over the fourteen u32 words of bytes 0..56
uint64_t header_digest(const uint8_t *b) {
    uint64_t s = 0;
    for (uint32_t w = 0; w < 14; w++) s += digest_term(w, get32(b + 4 * w));
    return s;
}

}  // namespace

int Fd::reset() {
    const int r = fd >= 0 ? ::close(fd) : 0;
    fd = -1;
    return r;
}

void encode_header(const Header &h, uint8_t out[HEADER_BYTES]) {
    memset(out, 0, HEADER_BYTES);
    memcpy(out, MAGIC, 8);
    put32(out + 8, VERSION);
    put32(out + 12, h.dim);
    put64(out + 16, h.rows);
    put32(out + 24, h.chunk_rows);
    put32(out + 28, h.n_chunks);
    put64(out + 32, h.valid_rows);
    put64(out + 56, header_digest(out));
}

bool decode_header(const uint8_t in[HEADER_BYTES], Header *h, std::string *why) {
    if (memcmp(in, MAGIC, 8) != 0) return *why = "not an index file (wrong magic)", false;
    if (get32(in + 8) != VERSION) return *why = "index file version " + std::to_string(get32(in + 8)) + ", this library reads version 1", false;
    if (get64(in + 56) != header_digest(in)) return *why = "header digest mismatch", false;
    h->dim = get32(in + 12);
    h->rows = get64(in + 16);
    h->chunk_rows = get32(in + 24);
    h->n_chunks = get32(in + 28);
    h->valid_rows = get64(in + 32);
    for (int i = 40; i < 56; i++)
        if (in[i]) return *why = "reserved header bytes are not zero", false;
    if (h->dim == 0) return *why = "dim is 0", false;
    if (h->dim > MAX_DIM) return *why = "dim " + std::to_string(h->dim) + " is above the index's limit of 2^20", false;
    if (h->rows > MAX_ROWS) return *why = "row count " + std::to_string(h->rows) + " is above the index's limit", false;
    if (h->chunk_rows == 0) return *why = "chunk_rows is 0", false;
    if (h->n_chunks != chunk_count(h->rows, h->chunk_rows)) return *why = "n_chunks disagrees with rows and chunk_rows", false;
    if (h->valid_rows > h->rows) return *why = "valid_rows exceeds rows", false;
    return true;
}

bool read_all(int fd, void *dst, size_t n) {
    uint8_t *p = static_cast<uint8_t *>(dst);
    while (n) {
        const ssize_t got = ::read(fd, p, n);
        if (got < 0 && errno == EINTR) continue;
        if (got <= 0) return false;
        p += got;
        n -= (size_t)got;
    }
    return true;
}

bn_status open_checked(const char *path, Header *h, Fd *fd) {
    (void)fd->reset();
    Fd f;
    f.fd = ::open(path, O_RDONLY | O_CLOEXEC);
    if (f.fd < 0) return set_last_error(BN_ERR_MODEL_LOAD, std::string("cannot open ") + path + ": " + strerror(errno));
    struct stat sb;
    if (fstat(f.fd, &sb) != 0 || !S_ISREG(sb.st_mode)) return set_last_error(BN_ERR_MODEL_LOAD, std::string(path) + " is not a regular file");
    uint8_t raw[HEADER_BYTES];
    if ((uint64_t)sb.st_size < HEADER_BYTES || !read_all(f.fd, raw, HEADER_BYTES))
        return set_last_error(BN_ERR_MODEL_LOAD, std::string(path) + ": shorter than an index file header");
    std::string why;
    if (!decode_header(raw, h, &why)) return set_last_error(BN_ERR_MODEL_LOAD, std::string(path) + ": " + why);
    if ((uint64_t)sb.st_size != file_bytes(*h))
        return set_last_error(BN_ERR_MODEL_LOAD, std::string(path) + ": " + std::to_string(sb.st_size) + " bytes, the header asks for " +
                                                     std::to_string(file_bytes(*h)) + ((uint64_t)sb.st_size < file_bytes(*h) ? " (truncated)" : " (trailing bytes)"));
    fd->fd = f.fd;
    f.fd = -1;
    return BN_OK;
}

}  // namespace index_file
}  // namespace bn

extern "C" {

bn_status bn_index_file_info(const char *path, bn_index_file_info_t *out, size_t struct_size) {
    if (!path || !out) return bn::set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (struct_size < sizeof(bn_index_file_info_t)) return bn::set_last_error(BN_ERR_INVALID_ARG, "struct_size is smaller than bn_index_file_info_t");
    bn::index_file::Header h;
    bn::index_file::Fd fd;
    bn_status st = bn::index_file::open_checked(path, &h, &fd);
    if (st != BN_OK) return st;
    out->rows = h.rows;
    out->valid_rows = h.valid_rows;
    out->dim = h.dim;
    out->chunk_rows = h.chunk_rows;
    out->n_chunks = h.n_chunks;
    out->version = bn::index_file::VERSION;
    return BN_OK;
}

bn_status bn_index_file_verify(const char *path, uint64_t *first_bad_chunk) {
    using namespace bn::index_file;
    if (first_bad_chunk) *first_bad_chunk = UINT64_MAX;
    if (!path) return bn::set_last_error(BN_ERR_INVALID_ARG, "null path");
    Header h;
    Fd in;
    bn_status st = open_checked(path, &h, &in);
    if (st != BN_OK) return st;
    const int raw_fd = in.fd;
    const std::string name(path);
    std::vector<uint64_t> table(h.n_chunks);
    if (h.n_chunks && !read_all(raw_fd, table.data(), table.size() * sizeof(uint64_t))) return bn::set_last_error(BN_ERR_MODEL_LOAD, name + ": read failed in the digest table");

    // the payload as one stream of elements; u = row * dim + k runs with it
    std::vector<uint32_t> buf(1u << 18);
    uint64_t left = h.rows * h.dim, u = 0, row = 0, valid_rows = 0, chunk = 0, sum = 0, rows_in_chunk = 0;
    uint32_t k = 0;
    bool row_nonzero = false;
    uint64_t bad_digest = UINT64_MAX, bad_finite = UINT64_MAX;
    while (left) {
        const size_t n = (size_t)std::min<uint64_t>(left, buf.size());
        if (!read_all(raw_fd, buf.data(), n * sizeof(uint32_t))) return bn::set_last_error(BN_ERR_MODEL_LOAD, name + ": read failed in the payload");
        for (size_t i = 0; i < n; i++) {
            const uint32_t b = buf[i];
            sum += bn::digest_term(u++, b);
            row_nonzero = row_nonzero || !bn::digest_is_zero(b);
            if (!bn::digest_is_finite(b) && bad_finite == UINT64_MAX) bad_finite = chunk;
            if (++k < h.dim) continue;
            k = 0;
            row++;
            valid_rows += row_nonzero ? 1 : 0;
            row_nonzero = false;
            if (++rows_in_chunk == h.chunk_rows || row == h.rows) {
                if (sum != table[chunk] && bad_digest == UINT64_MAX) bad_digest = chunk;
                chunk++;
                sum = 0;
                rows_in_chunk = 0;
            }
        }
        left -= n;
    }
    if (bad_digest != UINT64_MAX) {
        if (first_bad_chunk) *first_bad_chunk = bad_digest;
        return bn::set_last_error(BN_ERR_MODEL_LOAD, name + ": digest mismatch in chunk " + std::to_string(bad_digest) + " of " + std::to_string(h.n_chunks));
    }
    if (bad_finite != UINT64_MAX) {
        if (first_bad_chunk) *first_bad_chunk = bad_finite;
        return bn::set_last_error(BN_ERR_MODEL_LOAD, name + ": non-finite element in chunk " + std::to_string(bad_finite));
    }
    if (valid_rows != h.valid_rows)
        return bn::set_last_error(BN_ERR_MODEL_LOAD, name + ": the header counts " + std::to_string(h.valid_rows) + " valid rows, the payload holds " + std::to_string(valid_rows));
    return BN_OK;
}

}  // extern "C"
