// pk_radix5 / pk_radix5_tw_k / pk_radix25 (bds_acq_pfa.h: the FMA-fused 5-point butterfly of the N-point row pass) against a
// double-precision DFT: 64 lanes x 4 random cases each, then the unit impulses and all-ones.  Prints the largest error relative to
// the largest output per form.  What this catches and the compiler cannot: a wrong op_sel / neg bit of the packed instructions.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast -Ibds-3-b1c-b2a-sdr-receiver_amd/csrc -Iinclude tools/probe/bfly5_check.hip -o /tmp/bfly5_check
#include <hip/hip_runtime.h>

#include <cmath>
#include <complex>
#include <cstdio>
#include <random>
#include <vector>

#include "bds_acq_pfa.h"
using namespace bds;

constexpr int NL = 64, NCASE = 4, NPT = 25;  // every case owns 25 points, the 5-point forms use the first five

// mode 0: pk_radix5, 1..4: pk_radix5_tw_k with w25(q0 p1), p1 = mode, 5: pk_radix25, 6: pk_radix25<true> (sums handed over)
__global__ void k(float2 *io, int mode, int ncase) {
    for (int c = 0; c < ncase; ++c) {
        float2 *p = io + ((size_t)c * NL + threadIdx.x) * NPT;
        v2f x[NPT];
#pragma unroll
        for (int i = 0; i < NPT; ++i) x[i] = to_v2f(p[i]);
        if (mode == 0) pfa::pk_radix5(x[0], x[1], x[2], x[3], x[4]);
        else if (mode == 1) pfa::pk_radix5_tw_k(x[0], x[1], x[2], x[3], x[4], pfa::w25(1), pfa::w25(2), pfa::w25(3), pfa::w25(4));
        else if (mode == 2) pfa::pk_radix5_tw_k(x[0], x[1], x[2], x[3], x[4], pfa::w25(2), pfa::w25(4), pfa::w25(6), pfa::w25(8));
        else if (mode == 3) pfa::pk_radix5_tw_k(x[0], x[1], x[2], x[3], x[4], pfa::w25(3), pfa::w25(6), pfa::w25(9), pfa::w25(12));
        else if (mode == 4) pfa::pk_radix5_tw_k(x[0], x[1], x[2], x[3], x[4], pfa::w25(4), pfa::w25(8), pfa::w25(12), pfa::w25(16));
        else if (mode == 5) pfa::pk_radix25(x);
        else {
#pragma unroll
            for (int q0 = 0; q0 < 5; ++q0) x[q0 + 20] = x[q0 + 5] + x[q0 + 20], x[q0 + 15] = x[q0 + 10] + x[q0 + 15];
            pfa::pk_radix25<true>(x);
        }
#pragma unroll
        for (int i = 0; i < NPT; ++i) p[i] = to_f2(x[i]);
    }
}

int main() {
    typedef std::complex<double> cd;
    const double tau = 6.283185307179586476925;
    std::mt19937 rng(5);
    std::normal_distribution<float> nd;
    // random cases, then one set of structured ones: lane l < 25: unit impulse at point l (times 0.6 - 0.8 j), lane 25: all ones
    std::vector<float2> x((size_t)(NCASE + 1) * NL * NPT), y(x.size());
    for (auto &e : x) e = make_float2(nd(rng), nd(rng));
    for (int l = 0; l < NL; ++l)
        for (int i = 0; i < NPT; ++i) {
            float2 &e = x[((size_t)NCASE * NL + l) * NPT + i];
            if (l < 25) e = i == l ? make_float2(0.6f, -0.8f) : make_float2(0.f, 0.f);
            else if (l == 25) e = make_float2(1.f, 0.f);
        }
    float2 *d_x = nullptr;
    if (hipMalloc(&d_x, sizeof(float2) * x.size()) != hipSuccess) return printf("hipMalloc failed\n"), 2;
    const char *names[7] = {"pk_radix5", "pk_radix5_tw_k<p1=1>", "pk_radix5_tw_k<p1=2>", "pk_radix5_tw_k<p1=3>", "pk_radix5_tw_k<p1=4>", "pk_radix25", "pk_radix25<summed>"};
    int bad = 0;
    for (int mode = 0; mode < 7; ++mode) {
        if (hipMemcpy(d_x, x.data(), sizeof(float2) * x.size(), hipMemcpyHostToDevice) != hipSuccess) return printf("copy failed\n"), 2;
        hipLaunchKernelGGL(k, dim3(1), dim3(NL), 0, 0, d_x, mode, NCASE + 1);
        if (hipMemcpy(y.data(), d_x, sizeof(float2) * x.size(), hipMemcpyDeviceToHost) != hipSuccess) return printf("kernel or copy failed\n"), 2;
        const int R = mode < 5 ? 5 : 25;
        for (int part = 0; part < 2; ++part) {  // random cases, structured cases
            double worst = 0, big = 0;
            for (int c = part ? NCASE : 0; c < (part ? NCASE + 1 : NCASE); ++c)
                for (int l = 0; l < NL; ++l) {
                    const size_t o = ((size_t)c * NL + l) * NPT;
                    for (int kk = 0; kk < R; ++kk) {
                        cd acc = 0;
                        for (int n = 0; n < R; ++n) {
                            cd v(x[o + n].x, x[o + n].y);
                            if (mode >= 1 && mode <= 4) v *= std::polar(1.0, tau * (n * mode) / 25.0);
                            acc += v * std::polar(1.0, tau * n * kk / (double)R);
                        }
                        // slot s of the 25-point forms holds output slot25_index(s)
                        int slot = kk;
                        if (R == 25)
                            for (int s = 0; s < 25; ++s)
                                if (pfa::slot25_index(s) == kk) slot = s;
                        worst = std::max(worst, std::abs(acc - cd(y[o + slot].x, y[o + slot].y)));
                        big = std::max(big, std::abs(acc));
                    }
                }
            printf("%-22s %-10s max |err| / max |X| = %.2e\n", names[mode], part ? "impulses" : "random", worst / big);
            if (!(worst / big <= 1e-6)) bad = 1;
        }
    }
    (void)hipFree(d_x);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
