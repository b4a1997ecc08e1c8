// Stand-alone run of the navigation field parser and merger (csrc/bds_nav.cpp, reached through bds_nav_fields) under
// AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU: random bit arrays of every page / message type, all-ones and
// all-zeros arrays, and sequences that mix them.  An ordinary executable; nothing is loaded into Python.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -Iinclude \
//       -Ibds-3-b1c-b2a-sdr-receiver_amd/csrc tools/nav_fields_check.cpp bds-3-b1c-b2a-sdr-receiver_amd/csrc/bds_nav.cpp \
//       -o /tmp/nav_fields_check && /tmp/nav_fields_check
//
// Exit status 0 and "nav_fields_check: ok" = no report and every invariant held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "bds_mi355x.h"

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static void set_bits(uint8_t *msg, int first, int last, unsigned value) {  // 1-based, most significant bit first
    for (int i = last; i >= first; --i, value >>= 1) {
        const int k = i - 1;
        msg[k >> 3] = (uint8_t)((msg[k >> 3] & ~(0x80u >> (k & 7))) | ((value & 1u) ? (0x80u >> (k & 7)) : 0u));
    }
}

static int n_nan(const bds_eph &e) {
    int n = 0;
#define X(name) n += std::isnan(e.name);
    BDS_EPH_FIELDS(X)
#undef X
    return n;
}

int main() {
    std::mt19937_64 rng(2024);
    for (int signal : {BDS_SIGNAL_B1C, BDS_SIGNAL_B2A}) {
        const bool b1c = signal == BDS_SIGNAL_B1C;
        const int bytes = b1c ? (BDS_NAV_BITS_B1C + 7) / 8 : BDS_NAV_BITS_B2A / 8;  // exactly the stride the entry accepts
        const std::vector<int> kinds = b1c ? std::vector<int>{1, 3, 0, 63} : std::vector<int>{10, 11, 30, 31, 32, 33, 34, 0, 63};
        bds_eph e;
        // single messages: heap blocks of exactly `bytes` bytes, so a read past the last bit is a report
        for (int kind : kinds)
            for (int trial = 0; trial < 500; ++trial) {
                std::vector<uint8_t> m(bytes);
                for (auto &b : m) b = (uint8_t)rng();
                const unsigned prn = (unsigned)(rng() % 64);
                set_bits(m.data(), 1, 6, prn);
                set_bits(m.data(), b1c ? 615 : 7, b1c ? 620 : 12, (unsigned)kind);
                std::memset(&e, 0xA5, sizeof e);
                e.size = sizeof e;
                const int rc = bds_nav_fields(signal, m.data(), 1, bytes, &e);
                EXPECT(rc == (prn >= 1 ? 1 : 0));
                EXPECT(e.flag == rc && e.n_entered == rc && e.size == sizeof e);
                if (rc) {
                    EXPECT(e.PRN == prn && e.SatType >= 0 && e.SatType <= 3);
                    EXPECT(b1c ? e.TOW == e.HOW * 3600 + e.SOH : !std::isnan(e.SOW));
                } else {
                    EXPECT(n_nan(e) == 66);  // every double still []
                }
            }
        // all ones (PRN 63, every signed field -1), all zeros (PRN 0: not entered), and the two in sequence
        std::vector<uint8_t> ones(bytes, 0xFF), zeros(bytes, 0), both(2 * (size_t)bytes, 0);
        e.size = sizeof e;
        EXPECT(bds_nav_fields(signal, ones.data(), 1, bytes, &e) == 1 && e.PRN == 63);
        EXPECT(b1c ? e.deltaA == -std::ldexp(1.0, -9) : e.idValid[7] == 63);
        EXPECT(bds_nav_fields(signal, zeros.data(), 1, bytes, &e) == 0 && e.flag == 0 && n_nan(e) == 66);
        std::memset(both.data() + bytes, 0xFF, bytes);
        EXPECT(bds_nav_fields(signal, both.data(), 2, bytes, &e) == 1 && e.n_entered == 1);
        // sequences: the first-frame gates, later pages / types
        for (int trial = 0; trial < 300; ++trial) {
            const int n = 1 + (int)(rng() % 6);
            std::vector<uint8_t> seq((size_t)n * bytes);
            for (auto &b : seq) b = (uint8_t)rng();
            int want = 0;
            for (int i = 0; i < n; ++i) {
                const unsigned prn = (unsigned)(rng() % 64);
                set_bits(seq.data() + (size_t)i * bytes, 1, 6, prn);
                set_bits(seq.data() + (size_t)i * bytes, b1c ? 615 : 7, b1c ? 620 : 12, (unsigned)kinds[rng() % kinds.size()]);
                want += prn >= 1;
            }
            e.size = sizeof e;
            EXPECT(bds_nav_fields(signal, seq.data(), n, bytes, &e) == want && e.n_entered == want);
        }
        // refusals
        e.size = 0;
        EXPECT(bds_nav_fields(signal, ones.data(), 1, bytes, &e) == BDS_ERR_ARG);
        e.size = sizeof e;
        EXPECT(bds_nav_fields(signal, ones.data(), 1, bytes - 1, &e) == BDS_ERR_ARG);
        EXPECT(bds_nav_fields(signal, nullptr, 1, bytes, &e) == BDS_ERR_ARG);
        EXPECT(bds_nav_fields(7, ones.data(), 1, bytes, &e) == BDS_ERR_ARG);
    }
    std::printf(failures ? "nav_fields_check: %d FAILED\n" : "nav_fields_check: ok\n", failures);
    return failures ? 1 : 0;
}
