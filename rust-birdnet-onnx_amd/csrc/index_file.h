// The index file format on the host (include/birdnet_hip.h, bn_index_save): header encode / decode, the size rule and the checked
// open that bn_index_file_info, bn_index_file_verify (index_file.cpp) and bn_index_load (index_io.hip) share.  No HIP include: this
// header and index_file.cpp compile without the runtime (tools/asan_index_file.cpp builds them alone under the sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/birdnet_hip.h"
#include "last_error.h"

namespace bn {
namespace index_file {
constexpr size_t HEADER_BYTES = 64;
constexpr uint32_t VERSION = 1;
constexpr uint64_t MAX_DIM = 1u << 20;               // bn_index_create's limits
constexpr uint64_t MAX_ROWS = 0xffffffffull - 64 - 1;  // 2^32 - 66: the largest capacity bn_index_create takes

// a file descriptor closed on every way out
struct Fd {
    int fd = -1;
    Fd() = default;
    Fd(const Fd &) = delete;
    Fd &operator=(const Fd &) = delete;
    ~Fd() { (void)reset(); }
    int reset();  // closes; close()'s result, 0 when nothing was open
};

struct Header {
    uint32_t dim = 0;
    uint64_t rows = 0;
    uint32_t chunk_rows = 1, n_chunks = 0;
    uint64_t valid_rows = 0;
};

inline uint32_t chunk_count(uint64_t rows, uint32_t chunk_rows) { return (uint32_t)((rows + chunk_rows - 1) / chunk_rows); }
inline uint64_t table_offset() { return HEADER_BYTES; }
inline uint64_t payload_offset(const Header &h) { return HEADER_BYTES + 8ull * h.n_chunks; }
inline uint64_t file_bytes(const Header &h) { return payload_offset(h) + 4ull * h.rows * h.dim; }
// chunk_rows == 0 of bn_index_save: max(1, 2^21 / dim) rows, chunks of about 8 MB
inline size_t default_chunk_rows(size_t dim) { return dim >= (1u << 21) ? 1 : (size_t)(1u << 21) / dim; }

void encode_header(const Header &h, uint8_t out[HEADER_BYTES]);  // digest included
// false + *why for a wrong magic, version, header digest or a field outside the format's / the index's limits
bool decode_header(const uint8_t in[HEADER_BYTES], Header *h, std::string *why);
// opens `path` for reading, decodes the header and compares the file's size with the header's; BN_ERR_MODEL_LOAD (message set, nothing
// left open) for an unreadable or malformed file.  *fd is positioned behind the header
bn_status open_checked(const char *path, Header *h, Fd *fd);
// reads exactly n bytes at the descriptor's position (EINTR and short reads handled); false at an error or the end of the file
bool read_all(int fd, void *dst, size_t n);
}  // namespace index_file
}  // namespace bn
