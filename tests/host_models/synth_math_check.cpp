// Host build of csrc/bds_synth_math.h for tests/test_synth_cases.py: prints what the header computes -- the three published
// Philox4x32-10 answers, then words / uniforms of (seed, n) cases and symbols of (seed, period, prn, component) cases read from
// stdin -- for the test to hold against the NumPy restatement (tests/synth_cases.py).  No arithmetic of its own.
//   input lines:  "N seed n"  |  "S seed period prn component"      (seed unsigned, decimal)
//   output lines: "K w0 w1 w2 w3" (hex, three of them first) | "N w0 w1 w2 w3 u1bits u2bits" (hex) | "S symbol"
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "bds_synth_math.h"

static uint64_t bits(double x) {
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return u;
}

int main() {
    using namespace bds::synth;
    uint32_t w[4];
    philox4x32_10(0, 0, 0, 0, 0, 0, w);
    printf("K %08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
    philox4x32_10(~0u, ~0u, ~0u, ~0u, ~0u, ~0u, w);
    printf("K %08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
    philox4x32_10(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, w);
    printf("K %08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
    char kind;
    while (scanf(" %c", &kind) == 1) {
        uint64_t seed;
        int64_t a;
        if (scanf("%" SCNu64 " %" SCNd64, &seed, &a) != 2) return 1;
        if (kind == 'N') {
            double u1, u2;
            philox4x32_10((uint32_t)(uint64_t)a, (uint32_t)((uint64_t)a >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
            noise_uniforms(seed, a, u1, u2);
            printf("N %08x %08x %08x %08x %016" PRIx64 " %016" PRIx64 "\n", w[0], w[1], w[2], w[3], bits(u1), bits(u2));
        } else if (kind == 'S') {
            int prn, comp;
            if (scanf("%d %d", &prn, &comp) != 2) return 1;
            printf("S %d\n", symbol(seed, a, prn, comp));
        } else {
            return 1;
        }
    }
    return 0;
}
