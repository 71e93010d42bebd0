// Host-only test of csrc/hostmem.h: the owners, the two replace helpers and the guard over a
// counting heap that can be told to fail the N-th allocation.  No HIP runtime, no GPU.
// Built with -fsanitize=address,undefined by tests/test_hostmem_cpu.py; the exit status is
// the number of failed checks plus the live allocations at exit (0 = pass).
#define FQ_HOSTMEM_NO_HIP
#include "../../flow-q-learning_amd/csrc/hostmem.h"

#include <cstdio>
#include <cstdlib>
#include <new>
#include <set>

namespace {

// Every kind of resource comes from one heap, so one counter covers all four owners.
struct Heap {
    static inline std::set<void*> live;
    static inline long allocs = 0, releases = 0, double_frees = 0;
    static inline long fail_at = 0;  // the fail_at-th allocation from now fails (0: none)
    using event_t = void*;
    using stream_t = void*;
    static const char* get(void** p, size_t bytes) {
        if (fail_at && --fail_at == 0) return "out of memory (injected)";
        *p = std::malloc(bytes ? bytes : 1);
        live.insert(*p);
        ++allocs;
        return nullptr;
    }
    static void put(void* p) {
        ++releases;
        if (!live.erase(p)) { ++double_frees; return; }
        std::free(p);
    }
    static const char* alloc(void** p, size_t bytes) { return get(p, bytes); }
    static void free(void* p) { put(p); }
    static const char* host_alloc(void** p, size_t bytes, unsigned) { return get(p, bytes); }
    static void host_free(void* p) { put(p); }
    static const char* event_create(event_t* e, unsigned) { return get(e, 1); }
    static void event_destroy(event_t e) { put(e); }
    static const char* stream_create(stream_t* s) { return get(s, 1); }
    static void stream_destroy(stream_t s) { put(s); }
};

using Dev = fq::DevBuf<float, Heap>;
using Pinned = fq::HostBuf<long long, Heap>;
using Ev = fq::Event<Heap>;
using St = fq::Stream<Heap>;

int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

// a handle in miniature: several owners of every kind, built in sequence
struct Handle {
    St stream;
    Ev ev[2];
    Dev a, b;
    Pinned stage;
    Dev c;
    static constexpr int kAllocs = 7;
    static constexpr size_t kBytes[kAllocs] = {1, 1, 1, 4 * 100, 4 * 7, 8 * 33, 4 * 5};
    void build() {
        stream = St::create();
        for (auto& e : ev) e = Ev(0u);
        a = Dev(100, "a");
        b = Dev(7, "b");
        stage = Pinned(33, 0u, "stage");
        c = Dev(5, "c");
    }
};

struct Data {  // a setter's target: owners and their size, empty by default
    Dev obs, act;
    long long rows = 0;
};
Data make_data(long long rows) {
    Data d;
    d.obs = Dev(rows * 3, "obs");
    d.act = Dev(rows * 2, "act");
    d.rows = rows;
    return d;
}

void test_moves() {
    const long r0 = Heap::releases;
    {
        Dev x(10);
        float* p = x;
        CHECK(p && x.get() == p && Heap::live.size() == 1);
        Dev y(std::move(x));  // move construction
        CHECK(!x && y.get() == p && Heap::live.size() == 1);
        Dev z(3);
        z = std::move(y);     // move assignment releases z's own buffer, once
        CHECK(!y && z.get() == p && Heap::live.size() == 1 && Heap::releases == r0 + 1);
        Dev& zr = z;
        z = std::move(zr);    // self-move-assignment keeps the buffer
        CHECK(z.get() == p && Heap::live.size() == 1 && Heap::releases == r0 + 1);
        CHECK(z + 2 == p + 2);  // the implicit conversion: pointer arithmetic on the owner
    }
    CHECK(Heap::live.empty() && Heap::releases == r0 + 2 && Heap::double_frees == 0);
    Pinned h(4, 0u);
    St s = St::create();
    Ev e(0u);
    CHECK(Heap::live.size() == 3);
    for (int i = 0; i < 2; ++i) {  // reset() twice is harmless
        h.reset();
        s.reset();
        e.reset();
        CHECK(Heap::live.empty() && !h && !s && !e);
    }
    CHECK(Heap::releases == r0 + 5 && Heap::double_frees == 0);
}

void test_fail_nth() {
    for (int n = 1; n <= Handle::kAllocs; ++n) {
        Heap::fail_at = n;
        bool threw = false;
        try {
            Handle h;
            h.build();
        } catch (const fq::Err& e) {
            threw = true;
            CHECK(e.code == FQLPOP_E_HIP);
            CHECK(e.msg.find("injected") != std::string::npos);
            if (n > 3)  // memory: the error names the bytes requested
                CHECK(e.msg.find("allocating " + std::to_string(Handle::kBytes[n - 1]) + " bytes") != std::string::npos);
        }
        CHECK(threw && Heap::live.empty() && Heap::fail_at == 0);
    }
    {
        Handle h;
        h.build();  // and with no failure
        CHECK((long)Heap::live.size() == Handle::kAllocs);
    }
    CHECK(Heap::live.empty() && Heap::double_frees == 0);
}

void test_replace() {
    Data d;
    fq::replace_released(d, [] { return make_data(10); });
    CHECK(d.rows == 10 && d.obs && d.act && Heap::live.size() == 2);
    for (int n = 1; n <= 2; ++n) {  // release-first: a failure leaves the empty state, nothing live
        fq::replace_released(d, [] { return make_data(10); });
        Heap::fail_at = n;
        bool threw = false;
        try {
            fq::replace_released(d, [] { return make_data(20); });
        } catch (const fq::Err&) {
            threw = true;
        }
        CHECK(threw && d.rows == 0 && !d.obs && !d.act && Heap::live.empty());
    }
    fq::replace_built(d, [] { return make_data(10); });
    float* const obs = d.obs;
    float* const act = d.act;
    obs[29] = 7.f;
    for (int n = 1; n <= 2; ++n) {  // build-then-move: a failure leaves the previous contents
        Heap::fail_at = n;
        bool threw = false;
        try {
            fq::replace_built(d, [] { return make_data(20); });
        } catch (const fq::Err&) {
            threw = true;
        }
        CHECK(threw && d.rows == 10 && d.obs.get() == obs && d.act.get() == act && obs[29] == 7.f);
        CHECK(Heap::live.size() == 2);
    }
    fq::replace_built(d, [] { return make_data(20); });  // success: the old pair is released
    CHECK(d.rows == 20 && d.obs.get() != nullptr && Heap::live.size() == 2);
    d = Data{};
    CHECK(Heap::live.empty() && Heap::double_frees == 0);
}

void test_guard() {
    CHECK(fq::guard([] {}) == FQLPOP_OK && fq::g_last_error.empty());
    CHECK(fq::guard([] { throw fq::Err{FQLPOP_E_UNSUPPORTED, "not here"}; }) == FQLPOP_E_UNSUPPORTED);
    CHECK(fq::g_last_error == "not here");
    CHECK(fq::guard([] { ARGCHK(1 == 2, "bad argument"); }) == FQLPOP_E_ARG && fq::g_last_error == "bad argument");
    CHECK(fq::guard([] { throw std::bad_alloc(); }) == FQLPOP_E_STATE);
    CHECK(fq::g_last_error == std::bad_alloc().what());
    Heap::fail_at = 1;  // an owner's failure through the guard: the HIP code, the bytes in the text
    CHECK(fq::guard([] { Dev x(12, "x"); }) == FQLPOP_E_HIP);
    CHECK(fq::g_last_error.find("x: allocating 48 bytes failed") == 0);
    CHECK(fq::guard([] {}) == FQLPOP_OK && fq::g_last_error.empty());
}

}  // namespace

int main() {
    test_moves();
    test_fail_nth();
    test_replace();
    test_guard();
    std::printf("hostmem_test: %d failed checks, %zu live allocations, %ld allocations, %ld double frees\n", failures,
                Heap::live.size(), Heap::allocs, Heap::double_frees);
    return failures + (int)Heap::live.size() + (int)Heap::double_frees;
}
