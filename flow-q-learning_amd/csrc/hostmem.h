// Host-side plumbing of the C ABI: one error type, its check macros and guard, and move-only
// owners of device memory, mapped / pinned host memory, events and streams.  Every handle of
// the library is built on it, emtrain.hip (fqlpop_emtrain, fqlpop_initobs) and runtime.cpp
// (fqlpop, through the structs of popmem.h): every hipMalloc / hipFree / hipHostMalloc /
// hipHostFree and event and stream creation and destruction of those files is here.
//
// The owners take their back end (allocate / release) as one template policy, HipBackend by
// default; tests/cpp/hostmem_test.cpp (and emboot_test.cpp, popmem_test.cpp) define
// FQ_HOSTMEM_NO_HIP and run them over a counting heap that fails the N-th allocation.
#pragma once

#include <cstddef>
#include <exception>
#include <string>
#include <utility>

#include "../../include/fqlpop.h"
#ifndef FQ_HOSTMEM_NO_HIP
#include <hip/hip_runtime.h>
#endif

namespace fq {

struct Err {
    int code;
    std::string msg;
};

#define HIPCHK(x)                                                                                                    \
    do {                                                                                                             \
        if (hipError_t e_ = (x)) throw fq::Err{FQLPOP_E_HIP, std::string(#x) + " failed: " + hipGetErrorString(e_)}; \
    } while (0)
#define ARGCHK(c, m)                                           \
    do {                                                       \
        if (!(c)) throw fq::Err{FQLPOP_E_ARG, std::string(m)}; \
    } while (0)

// the text of the calling thread's last failed call ("" after a success)
inline thread_local std::string g_last_error;

// The body of every extern "C" entry point: no exception crosses the C ABI.
template <typename F>
int guard(F&& f) {
    try {
        f();
        g_last_error.clear();
        return FQLPOP_OK;
    } catch (const Err& e) {
        g_last_error = e.msg;
        return e.code;
    } catch (const std::exception& e) {
        g_last_error = e.what();
        return FQLPOP_E_STATE;
    }
}

#ifndef FQ_HOSTMEM_NO_HIP
// alloc / host_alloc return null on success, else the reason; the release calls ignore errors.
struct HipBackend {
    using event_t = hipEvent_t;
    using stream_t = hipStream_t;
    static const char* fail(hipError_t e) {
        if (e == hipSuccess) return nullptr;
        (void)hipGetLastError();
        return hipGetErrorString(e);
    }
    static const char* alloc(void** p, size_t bytes) { return fail(hipMalloc(p, bytes)); }
    static void free(void* p) { (void)hipFree(p); }
    static const char* host_alloc(void** p, size_t bytes, unsigned flags) { return fail(hipHostMalloc(p, bytes, flags)); }
    static void host_free(void* p) { (void)hipHostFree(p); }
    static const char* event_create(event_t* e, unsigned flags) { return fail(hipEventCreateWithFlags(e, flags)); }
    static void event_destroy(event_t e) { (void)hipEventDestroy(e); }
    static const char* stream_create(stream_t* s) { return fail(hipStreamCreateWithFlags(s, hipStreamNonBlocking)); }
    static void stream_destroy(stream_t s) { (void)hipStreamDestroy(s); }
};
using DefaultBackend = HipBackend;
#else
struct DefaultBackend;  // a host-only build names its back end in every owner type
#endif

// A move-only handle H released by Rel(h); a null handle owns nothing.
template <class H, auto Rel>
class Owned {
   public:
    Owned() = default;
    explicit Owned(H h) : h_(h) {}
    Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, H{})) {}
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) reset(std::exchange(o.h_, H{}));
        return *this;
    }
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { reset(); }
    H get() const { return h_; }
    operator H() const { return h_; }
    void reset(H h = H{}) {
        if (h_) Rel(h_);
        h_ = h;
    }

   private:
    H h_{};
};

// why: null, or the back end's reason why `what` failed
inline void made_check(const char* why, const std::string& what) {
    if (why) throw Err{FQLPOP_E_HIP, what + " failed: " + why};
}
inline std::string alloc_text(const char* what, size_t bytes) {
    return std::string(what) + ": allocating " + std::to_string(bytes) + " bytes";
}

// `count` elements of device memory (uninitialised); `what` names the buffer in the error text.
template <class T, class BE = DefaultBackend>
struct DevBuf : Owned<T*, &BE::free> {
    DevBuf() = default;
    explicit DevBuf(size_t count, const char* what = "device memory") {
        void* p = nullptr;
        made_check(BE::alloc(&p, sizeof(T) * count), alloc_text(what, sizeof(T) * count));
        this->reset(static_cast<T*>(p));
    }
};

// `count` elements of mapped / pinned host memory (hipHostMalloc flags).
template <class T, class BE = DefaultBackend>
struct HostBuf : Owned<T*, &BE::host_free> {
    HostBuf() = default;
    HostBuf(size_t count, unsigned flags, const char* what = "pinned host memory") {
        void* p = nullptr;
        made_check(BE::host_alloc(&p, sizeof(T) * count, flags), alloc_text(what, sizeof(T) * count));
        this->reset(static_cast<T*>(p));
    }
};

template <class BE = DefaultBackend>
struct Event : Owned<typename BE::event_t, &BE::event_destroy> {
    Event() = default;
    explicit Event(unsigned flags) {
        typename BE::event_t e{};
        made_check(BE::event_create(&e, flags), "event creation");
        this->reset(e);
    }
};

template <class BE = DefaultBackend>
struct Stream : Owned<typename BE::stream_t, &BE::stream_destroy> {
    Stream() = default;
    static Stream create() {  // a non-blocking stream
        Stream r;
        typename BE::stream_t s{};
        made_check(BE::stream_create(&s), "stream creation");
        r.reset(s);
        return r;
    }
};

// The two ways a setter replaces what a handle holds (T: a struct of owners and their sizes
// whose default-constructed value is the handle's documented empty state).
// Large buffers: released first, so peak memory does not rise; a failed build leaves `dst` empty.
template <class T, class F>
void replace_released(T& dst, F&& build) {
    dst = T{};
    dst = build();
}
// Small buffers: built aside and moved in on success; a failed build leaves `dst` as it was.
template <class T, class F>
void replace_built(T& dst, F&& build) {
    T fresh = build();
    dst = std::move(fresh);
}

}  // namespace fq
