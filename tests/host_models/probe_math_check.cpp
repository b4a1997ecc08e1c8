// Host build of csrc/bds_probe_math.h for tests/test_probedata_cases.py, run under AddressSanitizer + UndefinedBehaviorSanitizer:
// prints what the header computes for the test to hold against the NumPy restatement (tests/probedata_cases.py).  No arithmetic
// of its own.
//   output: "W sum_w2 w[0] w[1] w[16383] w[32767]"   the window (%.17g, the fp32 entries widened)
//           "T re im" x 3                             twiddles exp(-2 pi i m / 32768), m = 1, 8192, 32767 (fp32 entries)
//   input lines and the output line of each:
//     "P fmt n seg_per_piece"   ->  "P K n_pieces" then per piece "p seg0 seg1 hist0 hist1 load0 load1 byte0 byte1"
//     "A fmt n_bytes n_time cap has_q has_ex"  ->  "A rc n_samples"      check_args
//     "F ncase"  -> finish_psd on a ramp: "F fmt psd[0] psd[1] psd[last]" for fmt 0 and 1
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "bds_probe_math.h"

int main() {
    using namespace bds::probe;
    std::vector<float> w, t;
    const double s2 = window(w);
    printf("W %.17g %.17g %.17g %.17g %.17g\n", s2, (double)w[0], (double)w[1], (double)w[16383], (double)w[32767]);
    twiddles(kNfft, kNfft, t);
    for (int m : {1, 8192, 32767}) printf("T %.17g %.17g\n", (double)t[2 * m], (double)t[2 * m + 1]);
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'P') {
            int fmt;
            int64_t n, spp;
            if (scanf("%d %" SCNd64 " %" SCNd64, &fmt, &n, &spp) != 3) return 1;
            spp = default_piece_segments(fmt, spp);
            const int64_t np = piece_count(n, spp);
            printf("P %" PRId64 " %" PRId64 "\n", segments(n), np);
            for (int64_t j = 0; j < np; ++j) {
                const Piece p = piece(n, spp, j);
                int64_t b0, b1;
                byte_span(fmt, p.load0, p.load1, &b0, &b1);
                printf("p %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", p.seg0, p.seg1, p.hist0,
                       p.hist1, p.load0, p.load1, b0, b1);
            }
        } else if (kind == 'A') {
            int fmt, cap, has_q, has_ex;
            int64_t n_bytes, n_time, n = -7;
            if (scanf("%d %" SCNd64 " %" SCNd64 " %d %d %d", &fmt, &n_bytes, &n_time, &cap, &has_q, &has_ex) != 6) return 1;
            bds_settings s{};
            s.samplingFreq = 1.0;
            int64_t hist[2];
            double v[2];
            bds_probe_out o{};
            o.hist_i = hist, o.hist_q = has_q ? hist : nullptr, o.psd = v, o.cap = cap;
            o.excerpt_re = has_ex ? v : nullptr, o.excerpt_im = has_ex ? v : nullptr;
            char msg[200];
            const int rc = check_args(&s, fmt, n_bytes, 0, n_time, &o, &n, msg, sizeof msg);
            printf("A %d %" PRId64 " %s\n", rc, rc ? (int64_t)-1 : n, msg);
        } else if (kind == 'F') {
            int dummy;
            if (scanf("%d", &dummy) != 1) return 1;
            for (int fmt : {0, 1}) {
                const int nk2 = is_complex(fmt) ? kN2 : kN2 / 2 + 1;
                std::vector<double> acc((size_t)kN1 * nk2), psd(psd_bins(fmt));
                for (int k1 = 0; k1 < kN1; ++k1)
                    for (int k2 = 0; k2 < nk2; ++k2) acc[(size_t)k1 * nk2 + k2] = (double)(k1 + 8 * k2) + 1.0;  // bin k holds k + 1
                finish_psd(fmt, acc.data(), nk2, 4, 2.0, 8.0, psd.data());
                printf("F %d %.17g %.17g %.17g %.17g\n", fmt, psd[0], psd[1], psd[16384], psd.back());
            }
        } else {
            return 1;
        }
    }
    return 0;
}
