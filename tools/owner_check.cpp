// Host-side check of the resource owners (rust-birdnet-onnx_amd/csrc/device_mem.h; no device, no Python): the four owners over a
// runtime that only counts.  Handles are numbers that are never dereferenced; a release of a handle that is not live is an error.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__
//       -I/opt/rocm/include -Irust-birdnet-onnx_amd/csrc tools/owner_check.cpp -o /tmp/owner_check && /tmp/owner_check
// Exit 0 and "owner_check ok: N checks" when every check held.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <set>
#include <utility>
#include <vector>

#include "device_mem.h"

namespace {

struct Counting {
    static inline int calls = 0;     // acquiring calls so far
    static inline int fail_at = 0;   // the acquiring call (1-based) that fails; 0: none
    static inline int acquired = 0, released = 0, double_released = 0;
    static inline uintptr_t next = 0x1000;
    static inline std::set<uintptr_t> live;
    static inline std::vector<uintptr_t> release_order;

    static void restart(int fail = 0) {
        calls = acquired = released = double_released = 0;
        fail_at = fail;
        live.clear();
        release_order.clear();
    }
    static hipError_t acquire(uintptr_t *out) {
        if (++calls == fail_at) return hipErrorOutOfMemory;
        next += 0x100;
        live.insert(next);
        acquired++;
        *out = next;
        return hipSuccess;
    }
    static hipError_t give_back(uintptr_t h) {
        if (!live.erase(h)) double_released++;
        released++;
        release_order.push_back(h);
        return hipSuccess;
    }
    template <class H>
    static hipError_t acquire_as(H *out) {
        uintptr_t v = 0;
        hipError_t e = acquire(&v);
        if (e == hipSuccess) *out = reinterpret_cast<H>(v);
        return e;
    }
    static hipError_t device_alloc(void **p, size_t) { return acquire_as(p); }
    static hipError_t device_free(void *p) { return give_back(reinterpret_cast<uintptr_t>(p)); }
    static hipError_t host_alloc(void **p, size_t, unsigned) { return acquire_as(p); }
    static hipError_t host_free(void *p) { return give_back(reinterpret_cast<uintptr_t>(p)); }
    static hipError_t stream_create(hipStream_t *s, unsigned) { return acquire_as(s); }
    static inline int prio_creates = 0, last_prio = 0;
    static hipError_t stream_create_prio(hipStream_t *s, unsigned, int priority) {
        hipError_t e = acquire_as(s);
        if (e == hipSuccess) prio_creates++, last_prio = priority;
        return e;
    }
    static hipError_t stream_destroy(hipStream_t s) { return give_back(reinterpret_cast<uintptr_t>(s)); }
    static hipError_t event_create(hipEvent_t *e, unsigned) { return acquire_as(e); }
    static hipError_t event_destroy(hipEvent_t e) { return give_back(reinterpret_cast<uintptr_t>(e)); }
};

using Dev = bn::DeviceBuf<float, Counting>;
using Pin = bn::PinnedBuf<float, Counting>;
using Str = bn::StreamOf<Counting>;
using Evt = bn::EventOf<Counting>;
struct PrioStr : Str {};  // the same owner, acquired through create(flags, priority)

int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        g_checks++;                                                            \
        if (!(cond)) {                                                         \
            g_failed++;                                                        \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                      \
    } while (0)

bool balanced() { return Counting::acquired == Counting::released && Counting::double_released == 0 && Counting::live.empty(); }

hipError_t acquire(Dev &o) { return o.alloc(64); }
hipError_t acquire(Pin &o) { return o.alloc(64); }
hipError_t acquire(Str &o) { return o.create(hipStreamNonBlocking); }
hipError_t acquire(PrioStr &o) { return o.create(hipStreamNonBlocking, -1); }
hipError_t acquire(Evt &o) { return o.create(hipEventDisableTiming); }

// what every owner promises, whichever resource it holds
template <class O>
void check_owner() {
    Counting::restart();
    {
        O empty;
        CHECK(!empty.get());
    }
    CHECK(Counting::calls == 0 && Counting::released == 0);  // an empty owner releases nothing

    Counting::restart();
    {
        O a;
        CHECK(acquire(a) == hipSuccess && a.get());
        CHECK(a.get() == static_cast<decltype(a.get())>(a));  // the conversion is the handle
        CHECK(Counting::released == 0);
    }
    CHECK(Counting::acquired == 1 && Counting::released == 1 && balanced());  // scope exit: exactly once

    Counting::restart();
    {
        O a;
        CHECK(acquire(a) == hipSuccess);
        const auto h = a.get();
        O b(std::move(a));  // move construction
        CHECK(!a.get() && b.get() == h && Counting::released == 0);
        O c;
        c = std::move(b);  // move assignment into an empty owner
        CHECK(!b.get() && c.get() == h && Counting::released == 0);
        c = std::move(c);  // onto itself: nothing
        CHECK(c.get() == h && Counting::released == 0);
    }
    CHECK(Counting::acquired == 1 && Counting::released == 1 && balanced());  // the sources released nothing

    Counting::restart();
    {
        O a, b;
        CHECK(acquire(a) == hipSuccess && acquire(b) == hipSuccess);
        const auto old = a.get(), kept = b.get();
        a = std::move(b);  // over a live owner: the old value goes, once
        CHECK(Counting::released == 1 && Counting::release_order[0] == reinterpret_cast<uintptr_t>(old) && a.get() == kept && !b.get());
        CHECK(acquire(a) == hipSuccess);  // acquiring again releases what was held first
        CHECK(Counting::released == 2 && Counting::release_order[1] == reinterpret_cast<uintptr_t>(kept));
    }
    CHECK(Counting::acquired == 3 && Counting::released == 3 && balanced());

    Counting::restart();
    {
        O a;
        CHECK(acquire(a) == hipSuccess);
        a.reset();
        CHECK(!a.get() && Counting::released == 1);
        a.reset();  // idempotent
        a.reset();
        CHECK(Counting::released == 1);
    }
    CHECK(balanced());

    Counting::restart(1);
    {
        O a;
        CHECK(acquire(a) != hipSuccess && !a.get());  // a failed acquisition leaves the owner empty
    }
    CHECK(Counting::acquired == 0 && Counting::released == 0);

    Counting::restart(2);
    {
        O a;
        CHECK(acquire(a) == hipSuccess);
        CHECK(acquire(a) != hipSuccess && !a.get());  // over a live owner too: the old value went first
        CHECK(Counting::released == 1);
    }
    CHECK(balanced());

    Counting::restart();
    {
        O a;
        CHECK(acquire(a) == hipSuccess);
        const auto h = a.release();  // handed over: the owner forgets it
        CHECK(h && !a.get());
        a.reset();
        CHECK(Counting::released == 0);
        O b;
        CHECK(acquire(b) == hipSuccess);
    }
    CHECK(Counting::released == 1 && Counting::live.size() == 1);
}

// a handle shaped like a context: stream and event first, then the buffers their work touches
struct Ctx {
    Str stream;
    Evt done;
    Dev arena, input;
    Pin out;
    Dev scratch;
    static inline int waited_with_all_live = 0;
    ~Ctx() {  // the body runs before any member goes: whatever was acquired is still live while it waits
        size_t held = 0;
        for (const void *p : {(const void *)stream.get(), (const void *)done.get(), (const void *)arena.get(), (const void *)input.get(),
                              (const void *)out.get(), (const void *)scratch.get()})
            held += p ? 1 : 0;
        if (held == Counting::live.size()) waited_with_all_live++;
    }
};
#define TRY(expr)                          \
    do {                                   \
        hipError_t e_ = (expr);            \
        if (e_ != hipSuccess) return e_;   \
    } while (0)

// the shape of bn_ctx_create: six acquisitions, a return from the middle on the first failure, *out only on success
hipError_t ctx_create(Ctx **out) {
    *out = nullptr;
    auto c = std::make_unique<Ctx>();
    TRY(c->stream.create(hipStreamNonBlocking));
    TRY(c->arena.alloc(1 << 20));
    TRY(c->input.alloc(1 << 16));
    TRY(c->out.alloc(1 << 12));
    TRY(c->scratch.alloc(1 << 10));
    TRY(c->done.create(hipEventDisableTiming));
    *out = c.release();
    return hipSuccess;
}

void check_create_shape() {
    for (int fail = 1; fail <= 6; fail++) {
        Counting::restart(fail);
        Ctx::waited_with_all_live = 0;
        Ctx *c = nullptr;
        CHECK(ctx_create(&c) != hipSuccess && c == nullptr);
        CHECK(Counting::acquired == fail - 1 && Counting::released == fail - 1 && balanced());
        CHECK(Ctx::waited_with_all_live == 1);
    }
    Counting::restart();
    Ctx *c = nullptr;
    CHECK(ctx_create(&c) == hipSuccess && c != nullptr);
    CHECK(Counting::acquired == 6 && Counting::released == 0);
    // members go in reverse order of declaration: the stream, declared first, is the last to go
    const std::vector<uintptr_t> want = {reinterpret_cast<uintptr_t>(c->scratch.get()), reinterpret_cast<uintptr_t>(c->out.get()),
                                         reinterpret_cast<uintptr_t>(c->input.get()),   reinterpret_cast<uintptr_t>(c->arena.get()),
                                         reinterpret_cast<uintptr_t>(c->done.get()),    reinterpret_cast<uintptr_t>(c->stream.get())};
    delete c;
    CHECK(Counting::release_order == want);
    CHECK(Counting::released == 6 && balanced());
}

}  // namespace

int main() {
    check_owner<Dev>();
    check_owner<Pin>();
    check_owner<Str>();
    check_owner<Evt>();
    const int before = Counting::prio_creates;
    check_owner<PrioStr>();  // every promise again for a stream created at a priority level
    CHECK(Counting::prio_creates > before && Counting::last_prio == -1);
    Counting::restart();
    {
        Str s;  // one owner, both forms: each creation releases what the other left
        CHECK(s.create(hipStreamNonBlocking, -1) == hipSuccess && s.create(hipStreamNonBlocking) == hipSuccess);
        CHECK(Counting::released == 1 && s.create(hipStreamNonBlocking, 1) == hipSuccess && Counting::released == 2 && Counting::last_prio == 1);
    }
    CHECK(Counting::acquired == 3 && balanced());
    check_create_shape();
    // a typed buffer converts to its element pointer, so that arithmetic on it reads as on a raw member
    Counting::restart();
    {
        Dev d;
        CHECK(d.alloc(64) == hipSuccess);
        float *p = d;
        CHECK(d + 3 == p + 3 && static_cast<bool>(d));
    }
    CHECK(balanced());
    if (g_failed) return fprintf(stderr, "owner_check: %d of %d checks failed\n", g_failed, g_checks), 1;
    printf("owner_check ok: %d checks\n", g_checks);
    return 0;
}
