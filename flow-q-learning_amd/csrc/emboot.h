// The bootstrap tables of an env-model trainer handle (fqlpop_emtrain_set_bootstrap*): owners
// only, so that tests/cpp/emboot_test.cpp can run their life cycle (allocate, replace through
// a dataset change, drop, destroy) on the host over a counting heap, as hostmem_test.cpp does
// for hostmem.h.  The kernels that fill them are in emtrain.hip.
#pragma once

#include "hostmem.h"

namespace fq {

constexpr int EM_BOOT_MAX_MODELS = FQLPOP_EM_ENS_MAX_MODELS;

// K resamples of n_units units.  The default-constructed value is "bootstrap off".
template <class BE = DefaultBackend>
struct EmBootTables {
    DevBuf<long long, BE> table;        // [K][n_units] the unit a drawn index trains on
    DevBuf<long long, BE> oob;          // [K][n_units] the units table[k] misses, ascending
    DevBuf<long long, BE> n_oob;        // [K] their number
    DevBuf<unsigned char, BE> seen;     // [K][n_units] set-up scratch: unit occurs in table[k]
    DevBuf<float, BE> acc;              // [K][FQLPOP_EM_LOG_STRIDE] out-of-bag log sums
    long long n_units = 0;
    long long n_oob_h[EM_BOOT_MAX_MODELS] = {};  // n_oob on the host (refusals need no GPU call)

    explicit operator bool() const { return n_units > 0; }

    static EmBootTables make(int K, long long n_units) {
        EmBootTables b;
        const size_t n = (size_t)K * (size_t)n_units;
        b.table = DevBuf<long long, BE>(n, "bootstrap tables");
        b.oob = DevBuf<long long, BE>(n, "out-of-bag lists");
        b.n_oob = DevBuf<long long, BE>((size_t)K, "out-of-bag counts");
        b.seen = DevBuf<unsigned char, BE>(n, "bootstrap set-up flags");
        b.acc = DevBuf<float, BE>((size_t)K * FQLPOP_EM_LOG_STRIDE, "out-of-bag log sums");
        b.n_units = n_units;
        return b;
    }
};

// fqlpop_emtrain_set_dataset: the tables index the rows that go, so they go first; then the
// dataset as replace_released (a failed upload leaves no dataset and no tables).
template <class D, class B, class F>
void replace_dataset(D& data, B& boot, F&& build) {
    boot = B{};
    replace_released(data, std::forward<F>(build));
}

}  // namespace fq
