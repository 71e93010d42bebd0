// Host-only test of csrc/emboot.h: the life cycle of an env-model trainer's bootstrap tables
// (allocate, replace, replace the dataset under them, drop, destroy) over a counting heap that
// can be told to fail the N-th allocation, as hostmem_test.cpp does for the owners themselves.
// No HIP runtime, no GPU.  Built with -fsanitize=address,undefined by
// tests/test_emtrain_bootstrap_cpu.py; the exit status is the number of failed checks plus the
// live allocations and double frees at exit (0 = pass).
#define FQ_HOSTMEM_NO_HIP
#include "../../flow-q-learning_amd/csrc/emboot.h"

#include <cstdio>
#include <cstdlib>
#include <set>

namespace {

struct Heap {
    static inline std::set<void*> live;
    static inline long allocs = 0, double_frees = 0;
    static inline long fail_at = 0;  // the fail_at-th allocation from now fails (0: none)
    using event_t = void*;
    using stream_t = void*;
    static const char* alloc(void** p, size_t bytes) {
        if (fail_at && --fail_at == 0) return "out of memory (injected)";
        *p = std::malloc(bytes ? bytes : 1);
        live.insert(*p);
        ++allocs;
        return nullptr;
    }
    static void free(void* p) {
        if (!live.erase(p)) { ++double_frees; return; }
        std::free(p);
    }
    static const char* host_alloc(void** p, size_t bytes, unsigned) { return alloc(p, bytes); }
    static void host_free(void* p) { free(p); }
    static const char* event_create(event_t* e, unsigned) { return alloc(e, 1); }
    static void event_destroy(event_t e) { free(e); }
    static const char* stream_create(stream_t* s) { return alloc(s, 1); }
    static void stream_destroy(stream_t s) { free(s); }
};

using Boot = fq::EmBootTables<Heap>;
constexpr int kBootAllocs = 5;  // table, oob, n_oob, seen, acc

int failures = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

// the trainer handle in miniature: a dataset and the tables over its units
struct Data {
    fq::DevBuf<float, Heap> obs, rew;
    long long rows = 0;
};
Data make_data(long long rows) {
    Data d;
    d.obs = fq::DevBuf<float, Heap>(rows * 3, "obs");
    d.rew = fq::DevBuf<float, Heap>(rows, "rew");
    d.rows = rows;
    return d;
}
struct Handle {
    Data data;
    Boot boot;
};

// every byte of every table is the handle's to write
void touch(Boot& b, int K) {
    const long long n = b.n_units;
    for (long long i = 0; i < K * n; ++i) {
        b.table[i] = i % n;
        b.oob[i] = 0;
        b.seen[i] = 1;
    }
    for (int k = 0; k < K; ++k) b.n_oob[k] = b.n_oob_h[k] = 0;
    for (int i = 0; i < K * FQLPOP_EM_LOG_STRIDE; ++i) b.acc[i] = 0.f;
}

void test_allocate_drop_destroy() {
    {
        Handle h;
        CHECK(!h.boot && h.boot.n_units == 0 && Heap::live.empty());
        h.data = make_data(203);
        h.boot = Boot::make(3, 203);
        CHECK(h.boot && h.boot.n_units == 203 && (long)Heap::live.size() == 2 + kBootAllocs);
        touch(h.boot, 3);
        h.boot = Boot{};  // set_bootstrap(0): dropped, the dataset stays
        CHECK(!h.boot && !h.boot.table && !h.boot.oob && Heap::live.size() == 2);
        h.boot = Boot::make(16, 7);
        touch(h.boot, 16);
        CHECK((long)Heap::live.size() == 2 + kBootAllocs);
    }  // destroyed with tables
    CHECK(Heap::live.empty() && Heap::double_frees == 0);
}

void test_replace_keeps_the_earlier_tables_on_failure() {
    Handle h;
    h.data = make_data(20);
    fq::replace_built(h.boot, [] { return Boot::make(2, 20); });
    touch(h.boot, 2);
    long long* const table = h.boot.table;
    h.boot.n_oob_h[1] = 5;
    for (int n = 1; n <= kBootAllocs; ++n) {
        Heap::fail_at = n;
        bool threw = false;
        try {
            fq::replace_built(h.boot, [] { return Boot::make(2, 20); });
        } catch (const fq::Err& e) {
            threw = e.code == FQLPOP_E_HIP;
        }
        CHECK(threw && h.boot.table.get() == table && h.boot.n_units == 20 && h.boot.n_oob_h[1] == 5);
        CHECK((long)Heap::live.size() == 2 + kBootAllocs && Heap::fail_at == 0);
    }
    fq::replace_built(h.boot, [] { return Boot::make(2, 20); });  // success: the old set is released
    CHECK(h.boot.n_oob_h[1] == 0 && (long)Heap::live.size() == 2 + kBootAllocs);
}

void test_dataset_change_drops_the_tables() {
    Handle h;
    fq::replace_dataset(h.data, h.boot, [] { return make_data(10); });
    h.boot = Boot::make(3, 10);
    touch(h.boot, 3);
    fq::replace_dataset(h.data, h.boot, [] { return make_data(40); });
    CHECK(h.data.rows == 40 && !h.boot && !h.boot.table && Heap::live.size() == 2);
    h.boot = Boot::make(3, 40);
    touch(h.boot, 3);
    for (int n = 1; n <= 2; ++n) {  // a failed upload leaves no dataset and no tables
        Heap::fail_at = n;
        bool threw = false;
        try {
            fq::replace_dataset(h.data, h.boot, [] { return make_data(50); });
        } catch (const fq::Err&) {
            threw = true;
        }
        CHECK(threw && h.data.rows == 0 && !h.data.obs && !h.boot && Heap::live.empty());
        fq::replace_dataset(h.data, h.boot, [] { return make_data(40); });
        h.boot = Boot::make(3, 40);
    }
}

}  // namespace

int main() {
    test_allocate_drop_destroy();
    test_replace_keeps_the_earlier_tables_on_failure();
    test_dataset_change_drops_the_tables();
    std::printf("emboot_test: %d failed checks, %zu live allocations, %ld allocations, %ld double frees\n", failures,
                Heap::live.size(), Heap::allocs, Heap::double_frees);
    return failures + (int)Heap::live.size() + (int)Heap::double_frees;
}
