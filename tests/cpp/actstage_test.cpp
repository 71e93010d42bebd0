// Host-only test of csrc/popmem.h's PopActStage: the pinned host buffer and the device buffer
// fqlpop_act stages its observations, noise and results in, over a counting heap.  No HIP
// runtime, no GPU.  Built with -fsanitize=address,undefined by tests/test_act_cpu.py; the exit
// status is the failed checks plus the live allocations at exit plus the double frees.
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

constexpr int D = 3, A = 2;
using Stage = fq::PopActStage<Heap>;

bool empty(const Stage& s) { return s.cols == 0 && !s.host && !s.dev; }

// the runtime's use of the stage for a call of n <= cols columns: inputs from float 0, outputs
// from out_off(); every region written to its last float (ASan checks the ends)
void use(Stage& s, long long n, bool noise, bool out_noise) {
    for (float* buf : {s.host.get(), s.dev.get()}) {
        const size_t n_obs = (size_t)n * D, n_act = (size_t)n * A;
        std::memset(buf, 0, sizeof(float) * (n_obs + (noise ? n_act : 0)));
        std::memset(buf + s.out_off(), 0, sizeof(float) * n_act * (out_noise ? 2 : 1));
    }
}

void test_layout() {
    Stage s = Stage::make(7, D, A, 0u);
    CHECK(s.cols == 7 && s.D == D && s.A == A && s.out_off() == 7 * (D + A));
    CHECK(Heap::device_allocs == 1 && (int)Heap::live.size() == 2);
    for (size_t b : Heap::bytes_requested) CHECK(b == sizeof(float) * 7 * (D + 3 * A));
    use(s, 7, true, true);   // the full stage: inputs end where the outputs begin, outputs at the end
    use(s, 3, false, false);
    Stage moved = std::move(s);  // the owners move: nothing is copied or freed twice
    CHECK(!s.host && !s.dev && moved.host && moved.dev && (int)Heap::live.size() == 2);
}

void test_growth() {
    Stage s;
    CHECK(empty(s));
    for (int n = 1; n <= 2; ++n) {  // a failed growth leaves the documented empty state
        fq::replace_released(s, [] { return Stage::make(10, D, A, 0u); });
        CHECK(!empty(s) && (int)Heap::live.size() == 2);
        Heap::fail_at = n;
        bool threw = false;
        try {
            fq::replace_released(s, [] { return Stage::make(20, D, A, 0u); });
        } catch (const fq::Err& e) {
            threw = e.code == FQLPOP_E_HIP && e.msg.find("act stage") != std::string::npos;
        }
        Heap::fail_at = 0;
        CHECK(threw && empty(s) && Heap::live.empty());
    }
    fq::replace_released(s, [] { return Stage::make(10, D, A, 0u); });
    Heap::live_at_request.clear();
    fq::replace_released(s, [] { return Stage::make(20, D, A, 0u); });
    // the old buffers go before the first new allocation
    CHECK(Heap::live_at_request.front() == 0 && s.cols == 20 && (int)Heap::live.size() == 2);
    use(s, 20, true, true);
    s = Stage{};
    CHECK(empty(s) && Heap::live.empty() && Heap::double_frees == 0);
}

}  // namespace

int main() {
    test_layout();
    CHECK(Heap::live.empty());
    test_growth();
    std::printf("actstage_test: %d failed checks, %zu live allocations, %ld allocations, %ld double frees\n", failures,
                Heap::live.size(), Heap::allocs, Heap::double_frees);
    return failures + (int)Heap::live.size() + (int)Heap::double_frees;
}
