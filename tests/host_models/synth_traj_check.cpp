// Host build of the trajectory arithmetic of csrc/bds_synth_math.h (traj_index, traj_code, traj_carrier) for
// tests/test_synth_traj_cases.py: prints what the header computes for the cases read from stdin, for the test to hold against the
// NumPy restatement (tests/synth_traj_cases.py).  No arithmetic of its own.  Doubles travel as their bit patterns.
//   input lines:  "n first seg_log2 period0 code0 code1 code2 code3 carr0 carr1 carr2 carr3 phase"   (the last nine in hex)
//   output lines: "j u cph_bits period th_bits"                                                       (bits in hex)
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "bds_synth_math.h"

static uint64_t bits(double x) {
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return u;
}
static double dbl(uint64_t u) {
    double x;
    std::memcpy(&x, &u, 8);
    return x;
}

int main() {
    using namespace bds::synth;
    int64_t n, first, period0;
    int seg_log2;
    while (scanf("%" SCNd64 " %" SCNd64 " %d %" SCNd64, &n, &first, &seg_log2, &period0) == 4) {
        uint64_t h[9];
        for (uint64_t &v : h)
            if (scanf("%" SCNx64, &v) != 1) return 1;
        const double code[4] = {dbl(h[0]), dbl(h[1]), dbl(h[2]), dbl(h[3])}, carr[4] = {dbl(h[4]), dbl(h[5]), dbl(h[6]), dbl(h[7])};
        int64_t j, u, period;
        double cph;
        traj_index(n, first, seg_log2, j, u);
        traj_code(period0, code, (double)u, 10230.0, cph, period);
        const double th = traj_carrier(carr, (double)u, dbl(h[8]));
        printf("%" PRId64 " %" PRId64 " %016" PRIx64 " %" PRId64 " %016" PRIx64 "\n", j, u, bits(cph), period, bits(th));
    }
    return 0;
}
