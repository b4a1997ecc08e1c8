// The host arithmetic of the tone excisor (csrc/bds_notch_math.h) in a stand-alone program, so that it can run under the sanitizers
// (tests/test_notch_cases.py compiles it with -fsanitize=address,undefined).  Lines on stdin:
//   E sum r          -> estimate(sum, r); for r a power of two also estimate_full, which must agree
//   S e              -> sub_real(e) sub_cplx(e)
//   I step n         -> lo_index(phase(step, n))
//   A fmt n_bytes n_tones beta first cap step...   -> the return code of check_args and its message
//   P fmt piece beta -> piece_of
//   T                -> a checksum of the table (sum of C[i] (i + 1) and of S[i] (i + 1))
#include <cstdio>
#include <cstring>
#include <vector>

#include "bds_notch_math.h"

using namespace bds::notch;

int main() {
    char line[1024];
    while (std::fgets(line, sizeof line, stdin)) {
        long long a = 0, b = 0, c = 0;
        if (line[0] == 'E' && std::sscanf(line + 1, "%lld %lld", &a, &b) == 2) {
            const int32_t e = estimate(a, b);
            for (int beta = 0; beta <= 16; ++beta)
                if (b == ((long long)1 << beta) && estimate_full(a, beta) != e) return std::printf("estimate_full differs at %lld %lld\n", a, b), 1;
            std::printf("%d\n", e);
        } else if (line[0] == 'S' && std::sscanf(line + 1, "%lld", &a) == 1) {
            std::printf("%d %d\n", sub_real(a), sub_cplx(a));
        } else if (line[0] == 'I' && std::sscanf(line + 1, "%lld %lld", &a, &b) == 2) {
            std::printf("%u\n", lo_index(phase((uint32_t)a, b)));
        } else if (line[0] == 'A') {
            int fmt = 0, used = 0;
            long long n_bytes = 0, first = 0, cap = 0;
            bds_notch_opts o{};
            bds_notch_out r{};
            if (std::sscanf(line + 1, "%d %lld %d %d %lld %lld%n", &fmt, &n_bytes, &o.n_tones, &o.block_log2, &first, &cap, &used) != 6) return 2;
            const char *p = line + 1 + used;
            for (int k = 0; k < kMaxTones; ++k) {
                unsigned st = 0;
                int adv = 0;
                if (std::sscanf(p, "%u%n", &st, &adv) != 1) break;
                o.step[k] = st, p += adv;
            }
            std::vector<int32_t> est((size_t)(cap > 0 ? cap : 1) * 2);
            o.first_sample = first, o.apply = 1;
            if (cap >= 0) r.est = est.data(), r.est_cap = cap;
            char msg[256];
            int64_t n = -1;
            const int rc = check_args(fmt, n_bytes, 0, &o, &r, &n, msg, sizeof msg);
            std::printf("%d %lld %s\n", rc, (long long)n, msg);
        } else if (line[0] == 'P' && std::sscanf(line + 1, "%lld %lld %lld", &a, &b, &c) == 3) {
            std::printf("%lld\n", (long long)piece_of((int)a, b, (int)c));
        } else if (line[0] == 'T') {
            std::vector<int16_t> t((size_t)2 * kTab);
            lo_table(t.data());
            long long sc = 0, ss = 0;
            for (int i = 0; i < kTab; ++i) sc += (long long)t[i] * (i + 1), ss += (long long)t[kTab + i] * (i + 1);
            std::printf("%lld %lld\n", sc, ss);
        }
    }
    return 0;
}
