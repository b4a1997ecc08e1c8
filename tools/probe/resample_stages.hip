// Stage driver of the resampling conditioner (csrc/bds_resample.h) for tests/test_resample_stages_gpu.py: reads a case file written by
// tests/resample_cases.py (the format of tools/probe/pfa_stages.hip), launches the kernel each job names with the grid, the block and the
// dynamic LDS size condition_block of csrc/bds_acq.hip uses -- grid(2048), blk(256), 8 n_taps bytes -- and writes the raw device
// results to an output file.  No arithmetic of its own: inputs and references are Python's.  The kernels take n, nfact and n_taps at run
// time, so the driver runs shapes the library cannot reach.  Any HIP error ends the program with status 2; a malformed case, or one
// whose accesses would leave its buffers, with status 3 before any launch.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast -fno-slp-vectorize -I bds-3-b1c-b2a-sdr-receiver_amd/csrc -I include
//         tools/probe/resample_stages.hip -o resample_stages && ./resample_stages case.bin out.bin
//
// File format (both files, little endian): int64 count, then per array int64 byte length + the bytes (padded to 8).
// Case arrays: [0] int64 {magic, number of jobs}; then per job an int64 header and its inputs:
//   {1, nch, width (8 | 16), n, nfact};  int8 / int16 x[n][nch]                      k_ff_extend<nch, int8_t | int16_t>  -> double e[n + 2 nfact][nch]
//   {2, nch, len, n_taps, reverse};  double in[len][nch];  double b[n_taps]          k_ff_fir<nch>                       -> double out[len][nch]
//   {3, nch, nfact, sig_len, zlen};  double {new_fs, old_fs};  double z[zlen][nch]   k_ff_decimate<nch>                  -> double out[sig_len][nch]
//   {4, n};  int16 x[n]                                                             k_widen16                           -> double out[n]
// One result array per job: the output followed by a guard of kGuard doubles; output and guard are prefilled with the NaN kFill, so an
// element the kernel never wrote and a guard word it did write both show.  z has one prefilled element in front of it (what a
// decimation without its k = 0 rule would read at nfact = 0).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bds_resample.h"

using namespace bds;

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

constexpr int64_t kMagic = 0x52534D5053544147ll;  // "RSMPSTAG"
constexpr uint64_t kFill = 0x7FF8A5C31E870BD5ull;
constexpr size_t kGuard = 64;
constexpr int64_t kMaxLen = 1ll << 22;  // samples of one job
constexpr int kMaxTaps = 4096;          // 32 KB of LDS
static const dim3 kGrid(2048), kBlk(256);

typedef std::vector<unsigned char> Bytes;

static std::vector<Bytes> read_arrays(const char *path) {
    FILE *f = fopen(path, "rb");
    REQUIRE(f);
    int64_t n = 0;
    REQUIRE(fread(&n, 8, 1, f) == 1 && n > 0 && n < 16384);
    std::vector<Bytes> a((size_t)n);
    for (auto &b : a) {
        int64_t len = 0;
        REQUIRE(fread(&len, 8, 1, f) == 1 && len >= 0 && len < (1ll << 30));
        b.resize((size_t)((len + 7) / 8 * 8));
        REQUIRE(len == 0 || fread(b.data(), 1, b.size(), f) == b.size());
        b.resize((size_t)len);
    }
    fclose(f);
    return a;
}

struct Writer {
    FILE *f;
    int64_t n;
    void begin(int64_t count) {
        n = count;
        REQUIRE(fwrite(&n, 8, 1, f) == 1);
    }
    void add(const std::vector<uint64_t> &w) {
        const int64_t len = (int64_t)w.size() * 8;
        REQUIRE(fwrite(&len, 8, 1, f) == 1 && fwrite(w.data(), 8, w.size(), f) == w.size());
    }
};

// a device buffer of `front` + n + `back` doubles, all prefilled with kFill; returns the address of element 0 of the n
struct Filled {
    double *base = nullptr, *p = nullptr;
    size_t total = 0, front = 0;
    Filled(size_t n, size_t front_, size_t back) : total(front_ + n + back), front(front_) {
        CK(hipMalloc((void **)&base, total * 8));
        const std::vector<uint64_t> h(total, kFill);
        CK(hipMemcpy(base, h.data(), total * 8, hipMemcpyHostToDevice));
        p = base + front;
    }
    ~Filled() { (void)hipFree(base); }
    std::vector<uint64_t> download() const {  // the n elements and what is behind them
        std::vector<uint64_t> h(total - front);
        CK(hipMemcpy(h.data(), p, h.size() * 8, hipMemcpyDeviceToHost));
        return h;
    }
};

template <class T>
struct Upload {
    T *d = nullptr;
    explicit Upload(const Bytes &b) {
        CK(hipMalloc((void **)&d, b.size() ? b.size() : 8));
        if (!b.empty()) CK(hipMemcpy(d, b.data(), b.size(), hipMemcpyHostToDevice));
    }
    ~Upload() { (void)hipFree(d); }
};

static void finish(const Filled &out, Writer &w) {
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    w.add(out.download());
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: resample_stages case.bin out.bin\n");
        return 3;
    }
    const std::vector<Bytes> in = read_arrays(argv[1]);
    REQUIRE(in[0].size() == 16);
    const int64_t *H0 = (const int64_t *)in[0].data();
    REQUIRE(H0[0] == kMagic && H0[1] >= 1 && H0[1] < 8192);
    const int64_t njobs = H0[1];
    // ---- every job is checked before the first launch ----
    std::vector<size_t> at((size_t)njobs);
    size_t a = 1;
    for (int64_t j = 0; j < njobs; ++j) {
        at[(size_t)j] = a;
        REQUIRE(a < in.size() && in[a].size() >= 16 && in[a].size() % 8 == 0);
        const int64_t *H = (const int64_t *)in[a].data();
        const size_t nh = in[a].size() / 8;
        if (H[0] == 1) {
            REQUIRE(nh == 5 && a + 1 < in.size());
            const int64_t nch = H[1], width = H[2], n = H[3], nfact = H[4];
            REQUIRE((nch == 1 || nch == 2) && (width == 8 || width == 16) && nfact >= 0 && nfact < kMaxLen && n > nfact && n <= kMaxLen);  // (n > nfact: the reflections stay inside x)
            REQUIRE(in[a + 1].size() == (size_t)(n * nch * (width / 8)));
            a += 2;
        } else if (H[0] == 2) {
            REQUIRE(nh == 5 && a + 2 < in.size());
            const int64_t nch = H[1], len = H[2], n_taps = H[3], reverse = H[4];
            REQUIRE((nch == 1 || nch == 2) && len >= 1 && len <= kMaxLen && n_taps >= 1 && n_taps <= kMaxTaps && (reverse == 0 || reverse == 1));
            REQUIRE(in[a + 1].size() == (size_t)(len * nch * 8) && in[a + 2].size() == (size_t)(n_taps * 8));
            a += 3;
        } else if (H[0] == 3) {
            REQUIRE(nh == 5 && a + 2 < in.size());
            const int64_t nch = H[1], nfact = H[2], sig_len = H[3], zlen = H[4];
            REQUIRE((nch == 1 || nch == 2) && nfact >= 0 && nfact < kMaxLen && sig_len >= 1 && sig_len <= kMaxLen && zlen >= 1 && zlen <= 4 * kMaxLen);
            REQUIRE(in[a + 1].size() == 16 && in[a + 2].size() == (size_t)(zlen * nch * 8));
            const double new_fs = ((const double *)in[a + 1].data())[0], old_fs = ((const double *)in[a + 1].data())[1];
            REQUIRE(new_fs >= 1 && new_fs <= 1e12 && old_fs >= 1 && old_fs <= 1e12);
            // the index grows with k: the last one, with a sample to spare for another rounding, is inside z (the lowest, k = 0, reads
            // z[nfact] -- or the prefilled element in front of z[0], without the k = 0 rule at nfact = 0)
            REQUIRE((double)nfact + std::ceil((double)(sig_len - 1) / new_fs * old_fs) + 1.0 <= (double)zlen);
            a += 3;
        } else if (H[0] == 4) {
            REQUIRE(nh == 2 && a + 1 < in.size());
            REQUIRE(H[1] >= 1 && H[1] <= kMaxLen && in[a + 1].size() == (size_t)(H[1] * 2));
            a += 2;
        } else {
            REQUIRE(!"known stage");
        }
    }
    REQUIRE(a == in.size());
    Writer out{fopen(argv[2], "wb"), 0};
    REQUIRE(out.f);
    out.begin(njobs);
    for (int64_t j = 0; j < njobs; ++j) {
        a = at[(size_t)j];
        const int64_t *H = (const int64_t *)in[a].data();
        if (H[0] == 1) {
            const int nch = (int)H[1], width = (int)H[2], nfact = (int)H[4];
            const long n = (long)H[3];
            Upload<int8_t> x(in[a + 1]);
            Filled e((size_t)(n + 2L * nfact) * nch, 0, kGuard);
            if (width == 8 && nch == 1) hipLaunchKernelGGL((k_ff_extend<1, int8_t>), kGrid, kBlk, 0, 0, (const int8_t *)x.d, n, nfact, e.p);
            if (width == 8 && nch == 2) hipLaunchKernelGGL((k_ff_extend<2, int8_t>), kGrid, kBlk, 0, 0, (const int8_t *)x.d, n, nfact, e.p);
            if (width == 16 && nch == 1) hipLaunchKernelGGL((k_ff_extend<1, int16_t>), kGrid, kBlk, 0, 0, (const int16_t *)x.d, n, nfact, e.p);
            if (width == 16 && nch == 2) hipLaunchKernelGGL((k_ff_extend<2, int16_t>), kGrid, kBlk, 0, 0, (const int16_t *)x.d, n, nfact, e.p);
            finish(e, out);
        } else if (H[0] == 2) {
            const int nch = (int)H[1], n_taps = (int)H[3], reverse = (int)H[4];
            const long len = (long)H[2];
            Upload<double> u(in[a + 1]), b(in[a + 2]);
            Filled y((size_t)len * nch, 0, kGuard);
            if (nch == 1)
                hipLaunchKernelGGL(k_ff_fir<1>, kGrid, kBlk, sizeof(double) * n_taps, 0, (const double *)u.d, len, (const double *)b.d, n_taps, reverse, y.p);
            else
                hipLaunchKernelGGL(k_ff_fir<2>, kGrid, kBlk, sizeof(double) * n_taps, 0, (const double *)u.d, len, (const double *)b.d, n_taps, reverse, y.p);
            finish(y, out);
        } else if (H[0] == 3) {
            const int nch = (int)H[1], nfact = (int)H[2];
            const long sig_len = (long)H[3], zlen = (long)H[4];
            const double new_fs = ((const double *)in[a + 1].data())[0], old_fs = ((const double *)in[a + 1].data())[1];
            Filled z((size_t)zlen * nch, (size_t)nch, 0);
            CK(hipMemcpy(z.p, in[a + 2].data(), in[a + 2].size(), hipMemcpyHostToDevice));
            Filled y((size_t)sig_len * nch, 0, kGuard);
            if (nch == 1)
                hipLaunchKernelGGL(k_ff_decimate<1>, kGrid, kBlk, 0, 0, (const double *)z.p, nfact, sig_len, new_fs, old_fs, y.p);
            else
                hipLaunchKernelGGL(k_ff_decimate<2>, kGrid, kBlk, 0, 0, (const double *)z.p, nfact, sig_len, new_fs, old_fs, y.p);
            finish(y, out);
        } else {
            const long n = (long)H[1];
            Upload<int16_t> x(in[a + 1]);
            Filled y((size_t)n, 0, kGuard);
            hipLaunchKernelGGL(k_widen16, kGrid, kBlk, 0, 0, (const int16_t *)x.d, n, y.p);
            finish(y, out);
        }
    }
    CK(hipDeviceSynchronize());
    REQUIRE(fclose(out.f) == 0);
    printf("ok\n");
    return 0;
}
