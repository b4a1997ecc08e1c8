// Issue cycles of v_mfma_f32_16x16x16_f16 beside v_mfma_f32_16x16x32_f16 on one SIMD (gfx950), and what a second wave of the SIMD
// gets done meanwhile: (a) each form back to back on six independent accumulators, one and two waves per SIMD; (b) in a 512-thread
// workgroup -- waves w and w + 4 share a SIMD -- waves 0-3 issue matrix instructions only and waves 4-7 v_fma_f32 only, against each
// half running alone.  Times are shader-clock cycles (s_memtime) per wave, averaged over the waves of a role.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probe/mfma_k16.hip -o build/mfma_k16 && build/mfma_k16
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
constexpr int ITER = 1024;  // groups of 6 matrix instructions (or of 24 v_fma_f32)

#define FMA8 "v_fma_f32 %0, %0, %8, %9\n v_fma_f32 %1, %1, %8, %9\n v_fma_f32 %2, %2, %8, %9\n v_fma_f32 %3, %3, %8, %9\n" \
             "v_fma_f32 %4, %4, %8, %9\n v_fma_f32 %5, %5, %8, %9\n v_fma_f32 %6, %6, %8, %9\n v_fma_f32 %7, %7, %8, %9\n"

template <int K>
__device__ __forceinline__ void mfma6(f4 (&acc)[6], h8 a, h8 b) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        if (K == 32) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[i], 0, 0, 0);
        else acc[i] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_shufflevector(a, a, 0, 1, 2, 3), __builtin_shufflevector(b, b, 0, 1, 2, 3), acc[i], 0, 0, 0);
    }
}

// role of waves 0-3 / 4-7: 0 idle, 1 matrix (K), 2 v_fma_f32
template <int K>
__global__ __launch_bounds__(512) void k_probe(unsigned long long *out, float seed, int role_lo, int role_hi) {
    const int wave = threadIdx.x >> 6, role = wave < 4 ? role_lo : role_hi;
    h8 a, b;
    for (int i = 0; i < 8; ++i) a[i] = (_Float16)(seed + (threadIdx.x & 7) + i), b[i] = (_Float16)(seed * 0.5f + i);
    f4 acc[6];
    for (int i = 0; i < 6; ++i) acc[i] = (f4){seed, seed, seed, seed};
    float a0 = seed + threadIdx.x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7, b0 = seed * 0.5f, b1 = seed * 0.25f;
    __syncthreads();
    const unsigned long long t0 = __builtin_readcyclecounter();
    if (role == 1) {
        for (int it = 0; it < ITER / 4; ++it) {
            mfma6<K>(acc, a, b), mfma6<K>(acc, a, b), mfma6<K>(acc, a, b), mfma6<K>(acc, a, b);
        }
    } else if (role == 2) {
        for (int it = 0; it < ITER / 4; ++it) {
            asm volatile(FMA8 FMA8 FMA8 FMA8 FMA8 FMA8 FMA8 FMA8 FMA8 FMA8 FMA8 FMA8
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                         : "v"(b0), "v"(b1));
        }
    }
    float sink = 0.f;
    for (int i = 0; i < 6; ++i) sink += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    asm volatile("" ::"v"(sink));
    const unsigned long long t1 = __builtin_readcyclecounter();
    if ((threadIdx.x & 63) == 0) out[blockIdx.x * 8 + wave] = t1 - t0;
    if (sink + a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 == 1.2345f) out[0] = 0;
}

template <int K>
static void run(const char *name, unsigned long long *d_out, int role_lo, int role_hi) {
    const int grid = 256;
    std::vector<unsigned long long> h(grid * 8);
    for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(k_probe<K>, dim3(grid), dim3(512), 0, 0, d_out, 1.0f, role_lo, role_hi);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h.data(), d_out, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) {
        fprintf(stderr, "HIP error\n");
        exit(2);
    }
    double lo = 0, hi = 0;
    for (int b = 0; b < grid; ++b)
        for (int w = 0; w < 8; ++w) (w < 4 ? lo : hi) += (double)h[b * 8 + w];
    lo /= grid * 4.0 * ITER, hi /= grid * 4.0 * ITER;
    auto unit = [](int role) { return role == 1 ? 6.0 : role == 2 ? 24.0 : 1.0; };
    printf("%-44s waves 0-3: %8.2f cycles per group = %6.2f per instruction | waves 4-7: %8.2f per group = %6.2f per instruction\n", name, lo, lo / unit(role_lo), hi,
           hi / unit(role_hi));
}

int main() {
    unsigned long long *d_out;
    if (hipMalloc(&d_out, 256 * 8 * 8) != hipSuccess) return 2;
    run<32>("16x16x32 alone (one wave per SIMD)", d_out, 1, 0);
    run<16>("16x16x16 alone (one wave per SIMD)", d_out, 1, 0);
    run<32>("16x16x32 on both waves of a SIMD", d_out, 1, 1);
    run<16>("16x16x16 on both waves of a SIMD", d_out, 1, 1);
    run<32>("v_fma_f32 alone (one wave per SIMD)", d_out, 0, 2);
    run<32>("v_fma_f32 on both waves of a SIMD", d_out, 2, 2);
    run<32>("16x16x32 (waves 0-3) beside v_fma_f32 (4-7)", d_out, 1, 2);
    run<16>("16x16x16 (waves 0-3) beside v_fma_f32 (4-7)", d_out, 1, 2);
    run<32>("v_fma_f32 (waves 0-3) beside 16x16x32 (4-7)", d_out, 2, 1);
    return 0;
}
