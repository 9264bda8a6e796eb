// Host-side sanitizer check of what every search over an index shares before the device is involved (no device, no Python): the query
// source, the refusal of a query id that names no row, and the round arithmetic (rust-birdnet-onnx_amd/csrc/query_source.h).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Irust-birdnet-onnx_amd/csrc \
//       tools/asan_query_source.cpp -o /tmp/asan_query_source && /tmp/asan_query_source
// Exit 0: every refusal came with its text and names the first offending id, nothing is read of host rows or of an empty list, the
// rounds of every call are non-empty, in order, without gaps, no larger than the rows per round allow and sum to the call; nothing read
// memory it does not own and no arithmetic overflowed.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "query_source.h"

static std::string g_last;
// the library's definition lives in capi.cpp, which needs the runtime
bn_status bn::set_last_error(bn_status st, const std::string &msg) {
    g_last = msg;
    return st;
}

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) failures++, fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
    } while (0)

static bool refused(bn_status st, const std::string &text) { return st == BN_ERR_INVALID_ARG && g_last == text; }

using Rounds = std::vector<std::pair<size_t, size_t>>;
static Rounds rounds_of(size_t n, size_t rows, size_t unit) {
    Rounds r;
    EXPECT(bn::each_round(n, rows, unit, [&](size_t first, size_t count) {
               r.emplace_back(first, count);
               return BN_OK;
           }) == BN_OK);
    return r;
}

int main() {
    using bn::check_query_ids;
    using bn::IdLimit;
    using bn::QuerySource;
    // ---- the source: host rows carry no radius, whatever the caller of the _ids form would have passed
    {
        const float rows[4] = {};
        const uint64_t ids[2] = {};
        const QuerySource h = QuerySource::host(rows), s = QuerySource::stored(ids, 7), neg = QuerySource::stored(ids, -3);
        EXPECT(h.rows == rows && !h.ids && h.radius == -1 && h.data() == rows);
        EXPECT(!s.rows && s.ids == ids && s.radius == 7 && s.data() == ids);
        EXPECT(neg.radius == -3);  // a negative radius excludes nothing and is passed on as it is
        const QuerySource none = QuerySource::stored(nullptr, 7);
        EXPECT(!none.data() && none.radius == -1);
    }
    // ---- the id refusal: arrays of exactly the size named, so that a read past them is caught
    {
        const std::vector<uint64_t> ids{0, 99, 100, 5, 101};
        const QuerySource s = QuerySource::stored(ids.data(), 2);
        EXPECT(check_query_ids(s, 2, 100) == BN_OK && check_query_ids(s, 2, 100, IdLimit::VIEW) == BN_OK);
        EXPECT(check_query_ids(s, 0, 0) == BN_OK);                                    // n == 0: nothing is read
        EXPECT(check_query_ids(QuerySource::stored(nullptr, 2), 0, 0) == BN_OK);
        EXPECT(check_query_ids(s, 5, 102) == BN_OK);
        EXPECT(refused(check_query_ids(s, 3, 100), "query id 100 is not in the index"));  // an id equal to the limit
        EXPECT(refused(check_query_ids(s, 5, 100), "query id 100 is not in the index"));  // the first offender, not the largest
        EXPECT(refused(check_query_ids(s, 5, 100, IdLimit::VIEW), "query id 100 is not among the view's 100 rows"));
        EXPECT(refused(check_query_ids(s, 5, 101, IdLimit::VIEW), "query id 101 is not among the view's 101 rows"));
        EXPECT(refused(check_query_ids(s, 1, 0), "query id 0 is not in the index"));      // an empty index holds no id
        EXPECT(refused(check_query_ids(s, 1, 0, IdLimit::VIEW), "query id 0 is not among the view's 0 rows"));
        const std::vector<uint64_t> big{UINT64_MAX};
        EXPECT(refused(check_query_ids(QuerySource::stored(big.data(), 0), 1, 0xffffffffull - 65), "query id 18446744073709551615 is not in the index"));
        const std::vector<float> rows(8, 1.f);
        EXPECT(check_query_ids(QuerySource::host(rows.data()), 1000, 0) == BN_OK);     // host rows have no ids to refuse
    }
    // ---- the rounds
    size_t calls = 0;
    const size_t units[] = {1, 3, 64, 1024};
    const size_t ns[] = {0, 1, 341, 342, 1023, 1024, 1025, 2048, 2049};
    for (size_t unit : units)
        for (size_t n : ns) {
            const size_t per = 1024 / unit;
            const Rounds r = rounds_of(n, 1024, unit);
            calls++;
            EXPECT(r.size() == (n + per - 1) / per);
            size_t next = 0;
            for (size_t i = 0; i < r.size(); i++) {
                EXPECT(r[i].first == next && r[i].second >= 1 && r[i].second * unit <= 1024);
                EXPECT(i + 1 == r.size() || r[i].second == per);  // only the last round is short
                next += r[i].second;
            }
            EXPECT(next == n);
        }
    EXPECT(rounds_of(0, 1024, 1).empty());
    EXPECT((rounds_of(1, 1024, 1) == Rounds{{0, 1}}));
    EXPECT((rounds_of(1024, 1024, 1) == Rounds{{0, 1024}}));
    EXPECT((rounds_of(1025, 1024, 1) == Rounds{{0, 1024}, {1024, 1}}));
    EXPECT((rounds_of(2049, 1024, 1) == Rounds{{0, 1024}, {1024, 1024}, {2048, 1}}));
    EXPECT((rounds_of(400, 1024, 3) == Rounds{{0, 341}, {341, 59}}));  // 341 sequences of 3 windows fit 1024 rows
    EXPECT((rounds_of(3, 1024, 1024) == Rounds{{0, 1}, {1, 1}, {2, 1}}));
    for (size_t L = 1; L <= 64; L++) {  // the sequence search's units: as many as fit, never more
        const Rounds r = rounds_of(5000, 1024, L);
        EXPECT(!r.empty() && r[0].second * L <= 1024 && (r[0].second + 1) * L > 1024);
    }
    // a status that is not BN_OK ends the walk and is returned; a unit no round can hold is refused before anything runs
    {
        size_t seen = 0;
        const bn_status st = bn::each_round(5000, 1024, 1, [&](size_t first, size_t) { return ++seen, first >= 1024 ? BN_ERR_BACKEND : BN_OK; });
        EXPECT(st == BN_ERR_BACKEND && seen == 2);
        seen = 0;
        EXPECT(bn::each_round(1, 1024, 1025, [&](size_t, size_t) { return ++seen, BN_OK; }) == BN_ERR_INVALID_ARG && seen == 0);
        EXPECT(bn::each_round(1, 1024, 0, [&](size_t, size_t) { return ++seen, BN_OK; }) == BN_ERR_INVALID_ARG && seen == 0);
        EXPECT(bn::each_round(0, 1024, 0, [&](size_t, size_t) { return ++seen, BN_OK; }) == BN_OK && seen == 0);
    }
    printf("%zu calls, %d failures\n", calls, failures);
    return failures ? 1 : 0;
}
