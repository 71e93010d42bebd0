// Host-only test of csrc/popmem.h's PopRowStage: the mapped host buffers the rows of
// fqlpop_synth_write / fqlpop_synth_append wait in, over popmem_test.cpp's counting heap.  No
// HIP runtime, no GPU.  Built with -fsanitize=address,undefined by tests/test_synth_restore_cpu.py;
// the exit status is the failed checks plus the live allocations at exit plus the double frees.
#define FQ_HOSTMEM_NO_HIP
#include "../../flow-q-learning_amd/csrc/popmem.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

namespace {

struct Heap {
    static inline std::set<void*> live;
    static inline std::vector<size_t> live_at_request, bytes_requested;
    static inline long allocs = 0, double_frees = 0, device_allocs = 0;
    static inline long fail_at = 0;  // the fail_at-th allocation from now fails (0: none)
    using event_t = void*;
    using stream_t = void*;
    static const char* get(void** p, size_t bytes) {
        live_at_request.push_back(live.size());
        bytes_requested.push_back(bytes);
        if (fail_at && --fail_at == 0) return "out of memory (injected)";
        *p = std::malloc(bytes ? bytes : 1);  // exactly the bytes asked for: ASan guards the end
        live.insert(*p);
        ++allocs;
        return nullptr;
    }
    static void put(void* p) {
        if (!live.erase(p)) { ++double_frees; return; }
        std::free(p);
    }
    static const char* alloc(void** p, size_t bytes) { ++device_allocs; return get(p, bytes); }
    static void free(void* p) { put(p); }
    static const char* host_alloc(void** p, size_t bytes, unsigned) { return get(p, bytes); }
    static void host_free(void* p) { put(p); }
    static const char* event_create(event_t* e, unsigned) { return get(e, 1); }
    static void event_destroy(event_t e) { put(e); }
    static const char* stream_create(stream_t* s) { return get(s, 1); }
    static void stream_destroy(stream_t s) { put(s); }
};

int failures = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

constexpr int D = 3, A = 2, kStage = 2;
using Stage = fq::PopRowStage<kStage, Heap>;

bool empty(const Stage& s) {
    bool none = s.rows == 0;
    for (int i = 0; i < kStage; ++i) none = none && !s.host[i] && !s.used[i];
    return none;
}

// the runtime's packing of one call: field f of n rows at field(f, n), field_width(f) floats a row
void pack(const Stage& s, int stage, long long n, float tag) {
    float* hp = s.host[stage];
    for (int f = 0; f < 5; ++f) {
        std::vector<float> src((size_t)(n * s.field_width(f)), tag + (float)f);
        std::memcpy(hp + s.field(f, n), src.data(), sizeof(float) * src.size());
    }
}

void test_layout() {
    CHECK(Stage::width(D, A) == 2 * D + A + 2);
    Stage s = Stage::make(7, D, A, 0u);
    CHECK(s.rows == 7 && s.D == D && s.A == A && !s.used[0] && !s.used[1]);
    CHECK(Heap::device_allocs == 0 && (int)Heap::live.size() == kStage);
    for (size_t b : Heap::bytes_requested) CHECK(b == sizeof(float) * 7 * (2 * D + A + 2));
    const long long w[5] = {D, A, 1, 1, D};
    for (long long n : {1LL, 4LL, 7LL}) {  // the fields tile [0, n * width) in order, without gaps
        long long at = 0;
        for (int f = 0; f < 5; ++f) {
            CHECK(s.field(f, n) == at && s.field_width(f) == w[f]);
            at += n * w[f];
        }
        CHECK(at == n * Stage::width(D, A));
    }
    // a full buffer and a partial one, written to the last float (ASan checks the end) and read back
    pack(s, 0, 7, 10.0f);
    pack(s, 1, 4, 20.0f);
    for (int f = 0; f < 5; ++f) {
        CHECK(s.host[0][s.field(f, 7)] == 10.0f + f && s.host[0][s.field(f, 7) + 7 * w[f] - 1] == 10.0f + f);
        CHECK(s.host[1][s.field(f, 4)] == 20.0f + f && s.host[1][s.field(f, 4) + 4 * w[f] - 1] == 20.0f + f);
    }
    Stage moved = std::move(s);  // the owners move: nothing is copied or freed twice
    CHECK(!s.host[0] && !s.host[1] && moved.host[0][0] == 10.0f && (int)Heap::live.size() == kStage);
}

void test_growth() {
    Stage s;
    CHECK(empty(s));
    for (int n = 1; n <= kStage; ++n) {  // a failed growth leaves the documented empty state
        fq::replace_released(s, [] { return Stage::make(10, D, A, 0u); });
        CHECK(!empty(s) && (int)Heap::live.size() == kStage);
        s.used[1] = true;
        Heap::fail_at = n;
        bool threw = false;
        try {
            fq::replace_released(s, [] { return Stage::make(20, D, A, 0u); });
        } catch (const fq::Err& e) {
            threw = e.code == FQLPOP_E_HIP && e.msg.find("ring row stage") != std::string::npos;
        }
        Heap::fail_at = 0;
        CHECK(threw && empty(s) && Heap::live.empty());
    }
    fq::replace_released(s, [] { return Stage::make(10, D, A, 0u); });
    s.used[0] = true;
    Heap::live_at_request.clear();
    fq::replace_released(s, [] { return Stage::make(20, D, A, 0u); });
    // the old buffers go before the first new allocation, and a growth forgets their readers
    CHECK(Heap::live_at_request.front() == 0 && s.rows == 20 && !s.used[0] && (int)Heap::live.size() == kStage);
    pack(s, 0, 20, 1.0f);
    s = Stage{};
    CHECK(empty(s) && Heap::live.empty() && Heap::double_frees == 0);
}

}  // namespace

int main() {
    test_layout();
    CHECK(Heap::live.empty());
    test_growth();
    std::printf("rowstage_test: %d failed checks, %zu live allocations, %ld allocations, %ld double frees\n", failures,
                Heap::live.size(), Heap::allocs, Heap::double_frees);
    return failures + (int)Heap::live.size() + (int)Heap::double_frees;
}
