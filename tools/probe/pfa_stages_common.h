// What the four stage drivers of the N-point search pairs share (tools/probe/pfa_stages.hip, pfa32_stages.hip, pfa6_stages.hip,
// pfa31_stages.hip): the case-file reader and writer, the checks, the guarded buffers and the three stages.  A driver reads its own header
// fields, states its own shapes and names its plan (the `Plan` of its csrc/bds_acq_pfa*.h); every launch goes through that plan's
// forward / launch_rows / launch_cols -- the functions csrc/bds_acq.hip launches through -- with the case's grid and qchunk as their
// override parameters.  No arithmetic of its own: inputs and float64 references are Python's.  Any HIP error, a malformed case or a launch
// shape outside the buffers ends the program with a non-zero status.
//
// File format (both files, little endian): int64 count, then per array int64 byte length + the bytes (padded to 8).
// Case arrays: [0] int64 header {magic, stage, ...}; the rest per stage:
//   stage 1 (forward)  header {magic, 1, nb, doubled, conj, stride};  [1] double {scale};  [2] float2 x[nb][N]
//                      -> [0] uint32 dst (nb batches `stride` apart; doubled: every row stored twice)
//   stage 2 (rows, then optionally the column launches on the device's own buffer)
//                      header {magic, 2, ncells, gc, the driver's fields};  [1] uint32 Xs (signal spectra, rows doubled);
//                      [2] uint32 Cs[nslots][2][N];  [3] int32 bin[ncells];  [4] int64 cs[ncells];  [5] double launches[n][10 or 11]
//                      -> [0] uint32 guard | Bw (prefilled 0xff) | guard (if asked for, else the guards alone), then the launches' results
//   stage 3 (columns)  header {magic, 3, ncells};  [1] uint32 Bw[ncells][kCellElems];  [2] double launches[n][10 or 11]
// A column launch = {ncells, cell0, lb_div, qchunk, grid, extra_cap, stats?, keep, w0, w1 (, masked?)}; its results are five arrays:
//   uint64 cellmax[cell0 + ncells], float lb[cell0 + ncells], int32 {extra_count}, uint64 stats[4],
//   Extra guard (kGuardExtra) | the first min(count, cap) entries | guard behind the list's capacity
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bds_acq_sieve.h"

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

// a driver's way of raising a kernel's dynamic-LDS limit (the `lds` parameter of the plans' launchers)
static const auto set_lds = [](auto kern, size_t bytes) {
    CK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
};

// a case: its arrays, its header and the output file
struct Case {
    std::vector<Bytes> in;
    const int64_t *H;
    size_t nh;
    int stage;
    Writer out;
    Case(int argc, char **argv, const char *name) {
        if (argc != 3) {
            fprintf(stderr, "usage: %s case.bin out.bin\n", name);
            exit(3);
        }
        in = read_arrays(argv[1]);
        REQUIRE(in[0].size() >= 16);
        H = (const int64_t *)in[0].data();
        nh = in[0].size() / 8;
        REQUIRE(H[0] == kMagic);
        out = Writer{fopen(argv[2], "wb"), {}};
        REQUIRE(out.f);
        stage = (int)H[1];
    }
    int finish() {
        CK(hipDeviceSynchronize());
        out.flush();
        printf("ok\n");
        return 0;
    }
};

// stage 1: nb forward transforms of the case's x through Loader{x}.  shape_ok(nb, doubled, stride): the driver's bounds on them
template <class P, class Loader, class ShapeOk>
static void run_forward(Case &c, ShapeOk shape_ok) {
    REQUIRE(c.nh >= 6 && c.in.size() == 3 && c.in[1].size() == 8);
    const int nb = (int)c.H[2], doubled = (int)c.H[3], conj = (int)c.H[4];
    const long stride = (long)c.H[5];
    const float scale = (float)*(const double *)c.in[1].data();
    REQUIRE(shape_ok(nb, doubled, stride));
    REQUIRE(c.in[2].size() == (size_t)nb * P::NP * sizeof(float2));
    const size_t dst_elems = (size_t)(nb - 1) * stride + (doubled ? 2 * P::NP : P::NP);
    float2 *d_x = upload<float2>(c.in[2]), *d_tmp;
    uint32_t *d_dst;
    CK(hipMalloc((void **)&d_tmp, (size_t)2 * nb * P::NP * sizeof(float2)));
    CK(hipMalloc((void **)&d_dst, dst_elems * 4));
    CK(hipMemset(d_dst, 0xff, dst_elems * 4));
    P::forward(0, Loader{d_x}, nb, d_tmp, d_dst, stride, conj, scale, doubled);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<uint32_t> dst(dst_elems);
    CK(hipMemcpy(dst.data(), d_dst, dst_elems * 4, hipMemcpyDeviceToHost));
    c.out.add(dst.data(), dst_elems * 4);
}

// stage 2: the row pass of the case's cells into a guarded buffer; returns the device's inter-pass buffer for the column launches.
// xs_bytes: the size the driver's header gives the signal spectra; bin_ok(bin): the rotation of a cell stays below N; rows_args(ra):
// the driver's own fields on top of the RowsArgs every plan shares (Xs .. gc)
template <class P, class BinOk, class RowsArgsOf>
static const uint32_t *run_rows(Case &c, int ncells, int gc, int nslots, size_t guard, int write_bw, size_t xs_bytes, BinOk bin_ok, RowsArgsOf rows_args) {
    const std::vector<Bytes> &in = c.in;
    REQUIRE(ncells >= 1 && ncells <= 16 && gc >= 1 && nslots >= 1 && nslots <= 8 && guard >= 1024 && guard <= (1u << 22));
    REQUIRE(in[1].size() == xs_bytes && in[2].size() == (size_t)nslots * 2 * P::NP * 4);
    REQUIRE(in[3].size() == (size_t)ncells * 4 && in[4].size() == (size_t)ncells * 8);
    const int *bin = (const int *)in[3].data();
    const int64_t *cs = (const int64_t *)in[4].data();
    for (int i = 0; i < ncells; ++i) {  // what pfa_pick and the cell lists of csrc/bds_acq.hip guarantee
        REQUIRE(bin[i] >= 0 && bin_ok(bin[i]));
        REQUIRE(cs[i] >= 0 && cs[i] % (2 * P::NP) == 0 && cs[i] / (2 * P::NP) < nslots);
    }
    uint32_t *d_Xs = upload<uint32_t>(in[1]), *d_Cs = upload<uint32_t>(in[2]), *d_all;
    int *d_bin = upload<int>(in[3]);
    long *d_cs = upload<long>(in[4]);
    const size_t body = (size_t)ncells * P::kCellElems, total = body + 2 * guard;
    CK(hipMalloc((void **)&d_all, total * 4));
    fill_words(d_all, guard, kGuardWord);
    fill_words(d_all + guard + body, guard, kGuardWord);
    CK(hipMemset(d_all + guard, 0xff, body * 4));
    P::launch_rows(0, rows_args(typename P::RowsArgs{d_Xs, d_Cs, d_all + guard, d_bin, d_cs, ncells, gc}), (ncells + gc - 1) / gc, set_lds);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    if (write_bw) {
        std::vector<uint32_t> all(total);
        CK(hipMemcpy(all.data(), d_all, total * 4, hipMemcpyDeviceToHost));
        c.out.add(all.data(), total * 4);
    } else {  // the guards alone
        std::vector<uint32_t> g(2 * guard);
        CK(hipMemcpy(g.data(), d_all, guard * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(g.data() + guard, d_all + guard + body, guard * 4, hipMemcpyDeviceToHost));
        c.out.add(g.data(), g.size() * 4);
    }
    return d_all + guard;
}

// stage 3: the case's own inter-pass buffer
template <class P>
static const uint32_t *upload_cells(Case &c, size_t arrays, int *ncells) {
    REQUIRE(c.nh >= 3 && c.in.size() == arrays);
    *ncells = (int)c.H[2];
    REQUIRE(*ncells >= 1 && *ncells <= 16 && c.in[1].size() == (size_t)*ncells * P::kCellElems * 4);
    return upload<uint32_t>(c.in[1]);
}

// the column launches of a case (`width` doubles each) on the device's inter-pass buffer.  cols_args(p, ca): the driver's bound on the
// launch's cells (they lie inside the buffer) and its own fields on top of the ColsArgs every plan shares (Bw .. stats)
template <class P, class ColsArgsOf>
static void run_cols(const uint32_t *d_Bw, const Bytes &table, int width, ColsArgsOf cols_args, Writer &out) {
    REQUIRE(table.size() % (width * sizeof(double)) == 0);
    const int nl = (int)(table.size() / (width * sizeof(double)));
    if (!nl) return;
    const double *L = (const double *)table.data();
    uint4 *d_coef;
    CK(hipMalloc((void **)&d_coef, P::kCoefBytes));
    {
        std::vector<uint16_t> cf(P::kCoefBytes / 2);
        P::make_coef_frags(cf.data());
        CK(hipMemcpy(d_coef, cf.data(), P::kCoefBytes, hipMemcpyHostToDevice));
    }
    unsigned long long *d_stats;
    int *d_count;
    CK(hipMalloc((void **)&d_stats, 4 * sizeof(unsigned long long)));
    CK(hipMalloc((void **)&d_count, sizeof(int)));
    for (int l = 0; l < nl; ++l) {
        const double *p = L + width * l;
        const int ncells = (int)p[0], cell0 = (int)p[1], lb_div = (int)p[2], qchunk = (int)p[3], want_stats = (int)p[6];
        const long grid = (long)p[4], cap = (long)p[5];
        const float keep = (float)p[7], w0 = (float)p[8], w1 = (float)p[9];
        REQUIRE(ncells >= 1 && cell0 >= 0 && cell0 < 4096 && lb_div >= 1 && qchunk >= 1 && qchunk <= P::kTiles);
        REQUIRE(grid >= 1 && grid <= 65536 && cap >= 1 && cap <= (long)ncells * P::NP + 1024);
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
        typename P::ColsArgs ca{d_Bw, d_coef, ncells, w0, w1, {d_cellmax, d_lb, lb_div, d_extra + kGuardExtra, d_count, (int)cap, cell0, keep}, qchunk,
                                want_stats ? d_stats : nullptr};
        cols_args(p, ca);
        P::launch_cols(0, ca, qchunk, grid, set_lds);
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

// The whole driver of a plan on pfa::RowsArgs / pfa::ColsArgs (a whole number of spectrum bins per Doppler bin, no masked launch):
//   stage 2  header {magic, 2, ncells, gc, shift, nslots, guard elements, write Bw?}, launches of 10 doubles
// forward_shape_ok(nb, doubled, stride): the driver's bounds on stage 1
template <class P, class Loader, class ShapeOk>
static int stage_main(int argc, char **argv, const char *name, ShapeOk forward_shape_ok) {
    Case c(argc, argv, name);
    int ncells = 0;
    const auto cols_args = [&](const double *, typename P::ColsArgs &ca) {
        REQUIRE(ca.ncells <= ncells);
        ca.dbg_cell = ca.dbg_group = -1;
    };
    if (c.stage == 1) {
        run_forward<P, Loader>(c, forward_shape_ok);
    } else if (c.stage == 2) {
        REQUIRE(c.nh >= 8 && c.in.size() == 6);
        const int shift = (int)c.H[4];
        ncells = (int)c.H[2];
        REQUIRE(shift >= 1);
        const uint32_t *d_Bw = run_rows<P>(
            c, ncells, (int)c.H[3], (int)c.H[5], (size_t)c.H[6], (int)c.H[7], P::kSpecElems * 4, [&](int bin) { return (long)bin * shift < P::NP; },
            [&](typename P::RowsArgs ra) { return ra.shift = shift, ra; });
        run_cols<P>(d_Bw, c.in[5], 10, cols_args, c.out);
    } else if (c.stage == 3) {
        const uint32_t *d_Bw = upload_cells<P>(c, 3, &ncells);
        run_cols<P>(d_Bw, c.in[2], 10, cols_args, c.out);
    } else {
        REQUIRE(!"known stage");
    }
    return c.finish();
}
