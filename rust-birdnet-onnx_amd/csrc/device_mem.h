// Owners of the runtime's resources: a device buffer, a pinned host buffer, a stream, an event.  Each is empty by default, move-only,
// converts to the handle it holds (so launch sites and pointer arithmetic read as they did with raw members) and releases it in its
// destructor through the capture gate (hip_gate.h).  alloc / create release what was held first and leave the owner empty on
// failure; they return hipError_t, for BN_HIP_TRY.  No counting, no pooling: one owner, one resource.
//
// The order rule for a struct of owners: a destructor's body runs before its members go, and members go in reverse order of
// declaration.  So streams and events are declared BEFORE the buffers their work touches, and the body waits for them.
//
// The runtime calls come in as a policy, so that a host-only program can count them (tools/owner_check.cpp).
#pragma once
#include "hip_gate.h"

namespace bn {
struct GatedRuntime {
    static hipError_t device_alloc(void **p, size_t bytes) { return gated::Malloc(p, bytes); }
    static hipError_t device_free(void *p) { return gated::Free(p); }
    static hipError_t host_alloc(void **p, size_t bytes, unsigned flags) { return gated::HostMalloc(p, bytes, flags); }
    static hipError_t host_free(void *p) { return gated::HostFree(p); }
    static hipError_t stream_create(hipStream_t *s, unsigned flags) { return gated::StreamCreateWithFlags(s, flags); }
    static hipError_t stream_create_prio(hipStream_t *s, unsigned flags, int priority) { return gated::StreamCreateWithPriority(s, flags, priority); }
    static hipError_t stream_destroy(hipStream_t s) { return gated::StreamDestroy(s); }
    static hipError_t event_create(hipEvent_t *e, unsigned flags) { return gated::EventCreateWithFlags(e, flags); }
    static hipError_t event_destroy(hipEvent_t e) { return gated::EventDestroy(e); }
};

// what the four share: H is a pointer-like handle, Rel::release(H) gives it back
template <class H, class Rel>
class Owned {
   public:
    Owned() = default;
    Owned(Owned &&o) noexcept : h_(o.release()) {}
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) {
            reset();
            h_ = o.release();
        }
        return *this;
    }
    ~Owned() { reset(); }
    H get() const { return h_; }
    operator H() const { return h_; }
    H release() {  // the caller's from here on
        H h = h_;
        h_ = H{};
        return h;
    }
    void reset() {
        if (h_) (void)Rel::release(h_);
        h_ = H{};
    }

   protected:
    void adopt(H h) { h_ = h; }  // of an empty owner, after an acquiring call that succeeded

   private:
    H h_{};
};
template <class P>
struct DeviceRelease {
    static hipError_t release(const void *p) { return P::device_free(const_cast<void *>(p)); }
};
template <class P>
struct PinnedRelease {
    static hipError_t release(const void *p) { return P::host_free(const_cast<void *>(p)); }
};
template <class P>
struct StreamRelease {
    static hipError_t release(hipStream_t s) { return P::stream_destroy(s); }
};
template <class P>
struct EventRelease {
    static hipError_t release(hipEvent_t e) { return P::event_destroy(e); }
};

// sizes are in BYTES, as the allocation calls they replace took them
template <class T, class P = GatedRuntime>
struct DeviceBuf : Owned<T *, DeviceRelease<P>> {
    hipError_t alloc(size_t bytes) {
        this->reset();
        void *p = nullptr;
        hipError_t e = P::device_alloc(&p, bytes);
        if (e == hipSuccess) this->adopt(static_cast<T *>(p));
        return e;
    }
};
template <class T, class P = GatedRuntime>
struct PinnedBuf : Owned<T *, PinnedRelease<P>> {
    hipError_t alloc(size_t bytes, unsigned flags = hipHostMallocDefault) {
        this->reset();
        void *p = nullptr;
        hipError_t e = P::host_alloc(&p, bytes, flags);
        if (e == hipSuccess) this->adopt(static_cast<T *>(p));
        return e;
    }
};
template <class P = GatedRuntime>
struct StreamOf : Owned<hipStream_t, StreamRelease<P>> {
    hipError_t create(unsigned flags) {
        this->reset();
        hipStream_t s = nullptr;
        hipError_t e = P::stream_create(&s, flags);
        if (e == hipSuccess) this->adopt(s);
        return e;
    }
    // at a priority level of the device's range (hipDeviceGetStreamPriorityRange); released like any other stream
    hipError_t create(unsigned flags, int priority) {
        this->reset();
        hipStream_t s = nullptr;
        hipError_t e = P::stream_create_prio(&s, flags, priority);
        if (e == hipSuccess) this->adopt(s);
        return e;
    }
};
template <class P = GatedRuntime>
struct EventOf : Owned<hipEvent_t, EventRelease<P>> {
    hipError_t create(unsigned flags = hipEventDefault) {
        this->reset();
        hipEvent_t ev = nullptr;
        hipError_t e = P::event_create(&ev, flags);
        if (e == hipSuccess) this->adopt(ev);
        return e;
    }
};
using Stream = StreamOf<>;
using Event = EventOf<>;
}  // namespace bn
