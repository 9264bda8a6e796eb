// Host-side sanitizer check of the index file reader (no device, no Python): bn_index_file_info and bn_index_file_verify over a good
// file, every truncation of it and every single flipped byte of it (header, digest table and payload).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Irust-birdnet-onnx_amd/csrc \
//       tools/asan_index_file.cpp rust-birdnet-onnx_amd/csrc/index_file.cpp -o /tmp/asan_index_file
//   /tmp/asan_index_file good.bnindex scratch_dir       (a SMALL file: it is rewritten once per byte, twice)
// Exit 0: the good file passed both calls, every variant was refused by the verifier (and by info wherever the header or the size is
// what changed), and nothing read memory it does not own.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "index_file.h"

static std::string g_last;
// the library's definition lives in capi.cpp, which needs the runtime; the reader only reports through it
bn_status bn::set_last_error(bn_status st, const std::string &msg) {
    g_last = msg;
    return st;
}

static void write_file(const std::string &path, const std::vector<uint8_t> &bytes) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    f.write(reinterpret_cast<const char *>(bytes.data()), (std::streamsize)bytes.size());
}

int main(int argc, char **argv) {
    if (argc != 3) return fprintf(stderr, "usage: %s good_file scratch_dir\n", argv[0]), 2;
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> good((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const std::string variant = std::string(argv[2]) + "/variant.bnindex";
    bn_index_file_info_t info{};
    uint64_t bad = 0;
    if (bn_index_file_info(argv[1], &info, sizeof(info)) != BN_OK || bn_index_file_verify(argv[1], &bad) != BN_OK || bad != UINT64_MAX)
        return fprintf(stderr, "the good file was refused: %s\n", g_last.c_str()), 1;
    const size_t payload = bn::index_file::HEADER_BYTES + 8 * (size_t)info.n_chunks;
    printf("good: %zu bytes, dim %u, rows %llu, %u chunks\n", good.size(), info.dim, (unsigned long long)info.rows, info.n_chunks);
    if (bn_index_file_info((std::string(argv[2]) + "/missing").c_str(), &info, sizeof(info)) != BN_ERR_MODEL_LOAD) return fprintf(stderr, "a missing file was accepted\n"), 1;
    if (bn_index_file_info(argv[1], &info, sizeof(info) - 1) != BN_ERR_INVALID_ARG) return fprintf(stderr, "a short struct was accepted\n"), 1;

    int failures = 0;
    for (size_t cut = 0; cut < good.size(); cut++) {
        write_file(variant, std::vector<uint8_t>(good.begin(), good.begin() + cut));
        if (bn_index_file_info(variant.c_str(), &info, sizeof(info)) == BN_OK || bn_index_file_verify(variant.c_str(), nullptr) == BN_OK)
            failures++, fprintf(stderr, "truncation to %zu bytes was accepted\n", cut);
    }
    {
        std::vector<uint8_t> longer = good;
        longer.push_back(0);
        write_file(variant, longer);
        if (bn_index_file_info(variant.c_str(), &info, sizeof(info)) == BN_OK || bn_index_file_verify(variant.c_str(), nullptr) == BN_OK)
            failures++, fprintf(stderr, "a trailing byte was accepted\n");
    }
    for (const uint8_t mask : {(uint8_t)0x01, (uint8_t)0xff}) {
        for (size_t pos = 0; pos < good.size(); pos++) {
            std::vector<uint8_t> t = good;
            t[pos] ^= mask;
            write_file(variant, t);
            const bn_status si = bn_index_file_info(variant.c_str(), &info, sizeof(info));
            const bn_status sv = bn_index_file_verify(variant.c_str(), &bad);
            const bool in_header = pos < bn::index_file::HEADER_BYTES;
            if (sv == BN_OK || (in_header && si == BN_OK) || (!in_header && si != BN_OK))
                failures++, fprintf(stderr, "byte %zu ^ 0x%02x: info %d, verify %d\n", pos, mask, (int)si, (int)sv);
            if (!in_header && info.n_chunks && (bad == UINT64_MAX || bad >= info.n_chunks))
                failures++, fprintf(stderr, "byte %zu ^ 0x%02x (%s): no bad chunk named\n", pos, mask, pos < payload ? "table" : "payload");
        }
    }
    printf("%zu truncations, 1 extension, %zu flipped bytes: %d accepted or misreported\n", good.size(), 2 * good.size(), failures);
    return failures ? 1 : 0;
}
