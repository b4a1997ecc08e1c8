// Stage driver of the opt-in N-point search pair for B1C at 30.69 MS/s (csrc/bds_acq_pfa31.h) for tests/test_pfa31_stages_gpu.py: reads a
// case file written by tests/pfa31_cases.py (the format of tools/probe/pfa_stages.hip), launches the stage the case names exactly as
// csrc/bds_acq.hip launches it and writes the raw device results to an output file.  No arithmetic of its own: inputs and float64
// references are Python's.  Any HIP error, a malformed case or a launch shape outside the buffers ends the program with a non-zero status.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast -fno-slp-vectorize -I bds-3-b1c-b2a-sdr-receiver_amd/csrc
//         tools/probe/pfa31_stages.hip -o pfa31_stages && ./pfa31_stages case.bin out.bin
//
// File format (both files, little endian): int64 count, then per array int64 byte length + the bytes (padded to 8).
// Case arrays: [0] int64 header {magic, stage, ...}; the rest per stage:
//   stage 1 (forward)  header {magic, 1, nb, doubled, conj, stride};  [1] double {scale};  [2] float2 x[nb][N]
//                      -> [0] uint32 dst (nb batches `stride` apart; doubled: rows [31][11][3600], else [31][11][1800])
//   stage 2 (rows, then optionally the column launches on the device's own buffer)
//                      header {magic, 2, ncells, gc, shift, nslots, guard elements, write Bw?};  [1] uint32 Xs[31][11][3600];
//                      [2] uint32 Cs[nslots][2][N];  [3] int32 bin[ncells];  [4] int64 cs[ncells];  [5] double launches[n][10]
//                      -> [0] uint32 guard | Bw (prefilled 0xff) | guard (if asked for, else the guards alone), then the launches' results
//   stage 3 (columns)  header {magic, 3, ncells};  [1] uint32 Bw[ncells][kCellElems];  [2] double launches[n][10]
// A column launch = {ncells, cell0, lb_div, qchunk, grid, extra_cap, stats?, keep, w0, w1}.  Its results are five arrays:
//   uint64 cellmax[cell0 + ncells], float lb[cell0 + ncells], int32 {extra_count}, uint64 stats[4] ([0] wave items, [1] output blocks whose values were compared or listed),
//   Extra guard (kGuardExtra) | the first min(count, cap) entries | guard behind the list's capacity
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bds_acq_pfa31.h"

using namespace bds::pfa31;
using bds::pfa::ColsArgs;
using bds::pfa::RowsArgs;

#define CK(x)                                                                                  \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "HIP error %s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(2);                                                                           \
        }                                                                                      \
    } while (0)
#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "bad case %s:%d: %s\n", __FILE__, __LINE__, #c); \
            exit(3);                                                      \
        }                                                                 \
    } while (0)

constexpr int64_t kMagic = 0x5046415354414745ll;  // "PFASTAGE"
constexpr uint32_t kGuardWord = 0xA5C31E87u;
constexpr int kGuardExtra = 4096;  // entries in front of and behind the candidate list

struct ArrayLoader {  // the forward kernels' input: x[n] of transform `batch`
    const float2 *x;
    __device__ __forceinline__ float2 operator()(int batch, long n) const { return x[(size_t)batch * NP + n]; }
};

typedef std::vector<unsigned char> Bytes;

static std::vector<Bytes> read_arrays(const char *path) {
    FILE *f = fopen(path, "rb");
    REQUIRE(f);
    int64_t n = 0;
    REQUIRE(fread(&n, 8, 1, f) == 1 && n > 0 && n < 64);
    std::vector<Bytes> a((size_t)n);
    for (auto &b : a) {
        int64_t len = 0;
        REQUIRE(fread(&len, 8, 1, f) == 1 && len >= 0 && len < (1ll << 32));
        b.resize((size_t)((len + 7) / 8 * 8));
        REQUIRE(len == 0 || fread(b.data(), 1, b.size(), f) == b.size());
        b.resize((size_t)len);
    }
    fclose(f);
    return a;
}

struct Writer {
    FILE *f;
    std::vector<Bytes> arrays;
    void add(const void *p, size_t len) { arrays.emplace_back((const unsigned char *)p, (const unsigned char *)p + len); }
    void flush() {
        const int64_t n = (int64_t)arrays.size();
        REQUIRE(fwrite(&n, 8, 1, f) == 1);
        for (auto &b : arrays) {
            const int64_t len = (int64_t)b.size();
            b.resize((size_t)((len + 7) / 8 * 8));
            REQUIRE(fwrite(&len, 8, 1, f) == 1);
            REQUIRE(b.empty() || fwrite(b.data(), 1, b.size(), f) == b.size());
        }
        REQUIRE(fclose(f) == 0);
    }
};

template <class T>
static T *upload(const Bytes &b) {
    T *d = nullptr;
    CK(hipMalloc((void **)&d, b.size() ? b.size() : 8));
    if (!b.empty()) CK(hipMemcpy(d, b.data(), b.size(), hipMemcpyHostToDevice));
    return d;
}

static void fill_words(void *d, size_t words, uint32_t w) {
    std::vector<uint32_t> h(words, w);
    CK(hipMemcpy(d, h.data(), words * 4, hipMemcpyHostToDevice));
}

// the column launches of a case on the device's inter-pass buffer of `bw_cells` cells
static void run_cols(const uint32_t *d_Bw, int bw_cells, const Bytes &table, Writer &out) {
    REQUIRE(table.size() % (10 * sizeof(double)) == 0);
    const int nl = (int)(table.size() / (10 * sizeof(double)));
    if (!nl) return;
    const double *L = (const double *)table.data();
    uint4 *d_coef;
    CK(hipMalloc((void **)&d_coef, kCoefBytes));
    {
        std::vector<uint16_t> cf(kCoefBytes / 2);
        make_coef_frags(cf.data());
        CK(hipMemcpy(d_coef, cf.data(), kCoefBytes, hipMemcpyHostToDevice));
    }
    CK(hipFuncSetAttribute((const void *)k_pfa31_cols, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kColsLds));
    unsigned long long *d_stats;
    int *d_count;
    CK(hipMalloc((void **)&d_stats, 4 * sizeof(unsigned long long)));
    CK(hipMalloc((void **)&d_count, sizeof(int)));
    for (int l = 0; l < nl; ++l) {
        const double *p = L + 10 * l;
        const int ncells = (int)p[0], cell0 = (int)p[1], lb_div = (int)p[2], qchunk = (int)p[3], want_stats = (int)p[6];
        const long grid = (long)p[4], cap = (long)p[5];
        const float keep = (float)p[7], w0 = (float)p[8], w1 = (float)p[9];
        REQUIRE(ncells <= bw_cells);
        REQUIRE(ncells >= 1 && cell0 >= 0 && cell0 < 4096 && lb_div >= 1 && qchunk >= 1 && qchunk <= kTiles);
        REQUIRE(grid >= 1 && grid <= 65536 && cap >= 1 && cap <= (long)ncells * NP + 1024);
        const int slots = cell0 + ncells;
        unsigned long long *d_cellmax;
        float *d_lb;
        bds::Extra *d_extra;
        const size_t ex_total = (size_t)cap + 2 * kGuardExtra;
        CK(hipMalloc((void **)&d_cellmax, slots * sizeof(unsigned long long)));
        CK(hipMalloc((void **)&d_lb, slots * sizeof(float)));
        CK(hipMalloc((void **)&d_extra, ex_total * sizeof(bds::Extra)));
        CK(hipMemset(d_cellmax, 0, slots * sizeof(unsigned long long)));
        CK(hipMemset(d_lb, 0, slots * sizeof(float)));
        CK(hipMemset(d_count, 0, sizeof(int)));
        CK(hipMemset(d_stats, 0, 4 * sizeof(unsigned long long)));
        static_assert(sizeof(bds::Extra) == 12, "Extra is three words");
        fill_words(d_extra, (size_t)kGuardExtra * 3, kGuardWord);
        fill_words(d_extra + kGuardExtra + cap, (size_t)kGuardExtra * 3, kGuardWord);
        CK(hipMemset(d_extra + kGuardExtra, 0, (size_t)cap * sizeof(bds::Extra)));
        ColsArgs ca{d_Bw, d_coef, ncells, w0, w1, {d_cellmax, d_lb, lb_div, d_extra + kGuardExtra, d_count, (int)cap, cell0, keep}, qchunk,
                    want_stats ? d_stats : nullptr, nullptr, -1, -1};
        hipLaunchKernelGGL(k_pfa31_cols, dim3((unsigned)grid), dim3(kColsThreads), kColsLds, 0, ca);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        std::vector<unsigned long long> cm(slots), stats(4);
        std::vector<float> lb(slots);
        int count = 0;
        CK(hipMemcpy(cm.data(), d_cellmax, slots * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        CK(hipMemcpy(lb.data(), d_lb, slots * sizeof(float), hipMemcpyDeviceToHost));
        CK(hipMemcpy(&count, d_count, sizeof(int), hipMemcpyDeviceToHost));
        CK(hipMemcpy(stats.data(), d_stats, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        const size_t kept = count < 0 ? 0 : (size_t)(count < cap ? count : cap);
        std::vector<bds::Extra> ex((size_t)kGuardExtra + kept + kGuardExtra);
        CK(hipMemcpy(ex.data(), d_extra, ((size_t)kGuardExtra + kept) * sizeof(bds::Extra), hipMemcpyDeviceToHost));
        CK(hipMemcpy(ex.data() + kGuardExtra + kept, d_extra + kGuardExtra + cap, (size_t)kGuardExtra * sizeof(bds::Extra), hipMemcpyDeviceToHost));
        out.add(cm.data(), cm.size() * 8);
        out.add(lb.data(), lb.size() * 4);
        out.add(&count, 4);
        out.add(stats.data(), 32);
        out.add(ex.data(), ex.size() * sizeof(bds::Extra));
        CK(hipFree(d_cellmax));
        CK(hipFree(d_lb));
        CK(hipFree(d_extra));
    }
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: pfa31_stages case.bin out.bin\n");
        return 3;
    }
    const std::vector<Bytes> in = read_arrays(argv[1]);
    REQUIRE(in[0].size() >= 16);
    const int64_t *H = (const int64_t *)in[0].data();
    const size_t nh = in[0].size() / 8;
    REQUIRE(H[0] == kMagic);
    Writer out{fopen(argv[2], "wb"), {}};
    REQUIRE(out.f);
    const int stage = (int)H[1];
    if (stage == 1) {
        REQUIRE(nh >= 6 && in.size() == 3 && in[1].size() == 8);
        const int nb = (int)H[2], doubled = (int)H[3], conj = (int)H[4];
        const long stride = (long)H[5];
        const float scale = (float)*(const double *)in[1].data();
        const long per = doubled ? 2 * NP : NP;  // elements one transform stores
        REQUIRE(nb >= 1 && nb <= 2 && stride >= per && stride <= 4 * NP);
        REQUIRE(in[2].size() == (size_t)nb * NP * sizeof(float2));
        const size_t dst_elems = (size_t)(nb - 1) * stride + per;
        float2 *d_x = upload<float2>(in[2]), *d_tmp;
        uint32_t *d_dst;
        CK(hipMalloc((void **)&d_tmp, (size_t)2 * nb * NP * sizeof(float2)));
        CK(hipMalloc((void **)&d_dst, dst_elems * 4));
        CK(hipMemset(d_dst, 0xff, dst_elems * 4));
        forward(0, ArrayLoader{d_x}, nb, d_tmp, d_dst, stride, conj, scale, doubled);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        std::vector<uint32_t> dst(dst_elems);
        CK(hipMemcpy(dst.data(), d_dst, dst_elems * 4, hipMemcpyDeviceToHost));
        out.add(dst.data(), dst_elems * 4);
    } else if (stage == 2) {
        REQUIRE(nh >= 8 && in.size() == 6);
        const int ncells = (int)H[2], gc = (int)H[3], shift = (int)H[4], nslots = (int)H[5], write_bw = (int)H[7];
        const size_t guard = (size_t)H[6];
        REQUIRE(ncells >= 1 && ncells <= 16 && gc >= 1 && shift >= 1 && nslots >= 1 && nslots <= 8 && guard >= 1024 && guard <= (1u << 22));
        REQUIRE(in[1].size() == kSpecElems * 4 && in[2].size() == (size_t)nslots * 2 * NP * 4);
        REQUIRE(in[3].size() == (size_t)ncells * 4 && in[4].size() == (size_t)ncells * 8);
        const int *bin = (const int *)in[3].data();
        const int64_t *cs = (const int64_t *)in[4].data();
        for (int c = 0; c < ncells; ++c) {  // what pfa_pick and the cell lists of csrc/bds_acq.hip guarantee
            REQUIRE(bin[c] >= 0 && (long)bin[c] * shift < NP);
            REQUIRE(cs[c] >= 0 && cs[c] % (2 * NP) == 0 && cs[c] / (2 * NP) < nslots);
        }
        uint32_t *d_Xs = upload<uint32_t>(in[1]), *d_Cs = upload<uint32_t>(in[2]), *d_all;
        int *d_bin = upload<int>(in[3]);
        long *d_cs = upload<long>(in[4]);
        const size_t body = (size_t)ncells * kCellElems, total = body + 2 * guard;
        CK(hipMalloc((void **)&d_all, total * 4));
        fill_words(d_all, guard, kGuardWord);
        fill_words(d_all + guard + body, guard, kGuardWord);
        CK(hipMemset(d_all + guard, 0xff, body * 4));
        const int chunks = (ncells + gc - 1) / gc;
        RowsArgs ra{d_Xs, d_Cs, d_all + guard, d_bin, d_cs, ncells, gc, shift};
        CK(hipFuncSetAttribute((const void *)k_pfa31_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRowsLds));
        hipLaunchKernelGGL(k_pfa31_rows, dim3((unsigned)(kRowsWgs * chunks)), dim3(kRowsThreads), kRowsLds, 0, ra);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        if (write_bw) {
            std::vector<uint32_t> all(total);
            CK(hipMemcpy(all.data(), d_all, total * 4, hipMemcpyDeviceToHost));
            out.add(all.data(), total * 4);
        } else {  // the guards alone
            std::vector<uint32_t> g(2 * guard);
            CK(hipMemcpy(g.data(), d_all, guard * 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(g.data() + guard, d_all + guard + body, guard * 4, hipMemcpyDeviceToHost));
            out.add(g.data(), g.size() * 4);
        }
        run_cols(d_all + guard, ncells, in[5], out);
    } else if (stage == 3) {
        REQUIRE(nh >= 3 && in.size() == 3);
        const int ncells = (int)H[2];
        REQUIRE(ncells >= 1 && ncells <= 16 && in[1].size() == (size_t)ncells * kCellElems * 4);
        uint32_t *d_Bw = upload<uint32_t>(in[1]);
        run_cols(d_Bw, ncells, in[2], out);
    } else {
        REQUIRE(!"known stage");
    }
    CK(hipDeviceSynchronize());
    out.flush();
    printf("ok\n");
    return 0;
}
