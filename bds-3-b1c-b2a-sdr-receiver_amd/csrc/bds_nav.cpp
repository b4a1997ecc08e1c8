// Navigation decoding, host half: the BCH / CRC tables the kernels of bds_nav.hip read, the field parsers of
//   B1C/include/ephemeris.m:66-237   (B-CNAV1: one 878-bit decodedNav per frame)
//   B2a/include/ephemeris.m:60-310   (B-CNAV2: one 288-bit message)
// and the rules by which the decoding loops (BCNAV1decoding.m:176-188, BCNAV2decoding.m:141-157) merge frame after frame into
// one ephemeris.  Plain C++, no GPU: bds_nav_fields reaches all of it.
//
// Every scaled field is evaluated in the reference's order, (integer * 2^k) * pi in double; this file is compiled with
// -ffp-contract=off, and integer * 2^k is exact, so the one rounding is the multiplication by pi.
#include <cmath>
#include <cstddef>
#include <limits>

#include "bds_nav.h"

namespace bds {

namespace {

constexpr double kPi = 3.1415926535898;  // bdsPi / gpsPi (B1C/include/ephemeris.m:64, B2a/include/ephemeris.m:58)

// encoded(ind) = register(end); feedback = XOR of the register at the feedback positions; shift towards the end; register(1) =
// feedback (BCH21_6Decoding.m:82-89).  The register starts as the hypothesis, last element = its most significant bit (:68-79),
// so the first k symbols are the hypothesis itself.
uint64_t bch_encode(unsigned hyp, int k, int n, const int *fb, int n_fb) {
    int reg[8];
    for (int i = 0; i < k; ++i) reg[i] = (hyp >> i) & 1;  // fliplr of the MSB-first digits: reg[0] = least significant
    uint64_t cw = 0;
    for (int s = 0; s < n; ++s) {
        cw = (cw << 1) | (uint64_t)reg[k - 1];
        int f = 0;
        for (int j = 0; j < n_fb; ++j) f ^= reg[fb[j] - 1];
        for (int i = k - 1; i > 0; --i) reg[i] = reg[i - 1];
        reg[0] = f;
    }
    return cw;
}

NavTables make_tables() {
    NavTables t{};
    static const int fb21[] = {2, 4, 5, 6};        // BCH21_6Decoding.m:62
    static const int fb51[] = {1, 4, 5, 6, 7, 8};  // BCH51_8Decoding.m:60
    for (unsigned h = 0; h < 64; ++h) t.cw21[h] = (uint32_t)bch_encode(h, 6, 21, fb21, 4);
    for (unsigned h = 0; h < 256; ++h) t.cw51[h] = bch_encode(h, 8, 51, fb51, 6);
    uint32_t r = 1;
    for (int e = 0; e < 600; ++e) {
        t.crc[e] = r;
        r <<= 1;
        if (r & 0x1000000u) r ^= 0x1864CFBu;
    }
    return t;
}

// navBitsBin(first:last), 1-based, as an unsigned integer (bin2dec); at most 33 bits here
inline uint64_t ubits(const uint8_t *b, int first, int last) {
    uint64_t v = 0;
    for (int i = first - 1; i < last; ++i) v = (v << 1) | ((b[i >> 3] >> (7 - (i & 7))) & 1u);
    return v;
}
// twosComp2dec (Common/twosComp2dec.m:39-44)
inline int64_t sbits(const uint8_t *b, int first, int last) {
    const int w = last - first + 1;
    int64_t v = (int64_t)ubits(b, first, last);
    if (v >> (w - 1)) v -= (int64_t)1 << w;
    return v;
}

struct Field {
    size_t off;        // of the double in bds_eph
    short first, last; // navBitsBin(first:last)
    bool sgn;          // twosComp2dec (else bin2dec)
    double mul;        // the factor the reference multiplies by first (18, 300, 3, 2^k; 1 = none)
    bool pi;           // ... and then by pi
};
#define F(name, first, last, sgn, mul, pi) {offsetof(bds_eph, name), first, last, sgn, mul, pi}
inline double p2(int k) { return std::ldexp(1.0, k); }

void apply(const Field *f, size_t n, const uint8_t *b, bds_eph *e) {
    for (size_t i = 0; i < n; ++i) {
        double v = f[i].sgn ? (double)sbits(b, f[i].first, f[i].last) : (double)ubits(b, f[i].first, f[i].last);
        if (f[i].mul != 1.0) v = v * f[i].mul;
        if (f[i].pi) v = v * kPi;
        *reinterpret_cast<double *>(reinterpret_cast<char *>(e) + f[i].off) = v;
    }
}
template <size_t N>
void apply(const Field (&f)[N], const uint8_t *b, bds_eph *e) { apply(f, N, b, e); }

void sat_type(uint64_t code, bds_eph *e) {  // 0 leaves the field as it is (B1C/include/ephemeris.m:92-99, B2a: :96-103)
    if (code >= 1 && code <= 3) e->SatType = (int32_t)code;
}

// ---- B-CNAV1 (B1C/include/ephemeris.m), bit numbers of the 878-bit decodedNav -------------------------------------------------
int enter_b1c(const uint8_t *b, bds_eph *e) {
    const uint64_t prn = ubits(b, 1, 6);
    if (prn < 1 || prn > 63) return 0;  // :68-70 returns here; this library does not enter the frame (bds_mi355x.h)
    e->PRN = (double)prn;               // :67 stands before the flag gate: every entered frame sets it
    const bool first = !e->flag;
    if (first) {  // :72-161 (isempty(eph.flag)): SOH and sub-frame 2 from the first entered frame only
        static const Field f[] = {
            F(SOH, 7, 14, false, 18, false),  // :74
            // navBitsBin(15:53), :77-85
            F(WN, 15, 27, false, 1, false), F(HOW, 28, 35, false, 1, false), F(IODC, 36, 46, false, 1, false),
            F(IODE, 46, 53, false, 1, false),  // :85 reads 32:39 of the block: its first bit is IODC's last, as in the reference
            // ephemeris I, navBitsBin(54:256), :88-113
            F(t_oe, 54, 64, false, 300, false), F(deltaA, 67, 92, true, p2(-9), false), F(ADot, 93, 117, true, p2(-21), false),
            F(delta_n_0, 118, 134, true, p2(-44), true), F(delta_n_0Dot, 135, 157, true, p2(-57), true),
            F(M_0, 158, 190, true, p2(-32), true), F(e, 191, 223, false, p2(-34), false), F(omega, 224, 256, true, p2(-32), true),
            // ephemeris II, navBitsBin(257:478), :116-140
            F(omega_0, 257, 289, true, p2(-32), true), F(i_0, 290, 322, true, p2(-32), true),
            F(omegaDot, 323, 341, true, p2(-44), true), F(i_0Dot, 342, 356, true, p2(-44), true),
            F(C_is, 357, 372, true, p2(-30), false), F(C_ic, 373, 388, true, p2(-30), false), F(C_rs, 389, 412, true, p2(-8), false),
            F(C_rc, 413, 436, true, p2(-8), false), F(C_us, 437, 457, true, p2(-30), false), F(C_uc, 458, 478, true, p2(-30), false),
            // clock, navBitsBin(479:547), :143-151
            F(t_oc, 479, 489, false, 300, false), F(a_0, 490, 514, true, p2(-34), false), F(a_1, 515, 536, true, p2(-50), false),
            F(a_2, 537, 547, true, p2(-66), false),
            // group delays, navBitsBin(548:583), :154-160
            F(T_GDB2ap, 548, 559, true, p2(-34), false), F(ISC_B1Cd, 560, 571, true, p2(-34), false),
            F(T_GDB1Cp, 572, 583, true, p2(-34), false),
        };
        apply(f, b, e);
        sat_type(ubits(b, 65, 66), e);  // :92
    }
    // sub-frame 3, navBitsBin(615:878), from every entered frame (:164-230)
    static const Field f3[] = {
        F(HS, 621, 622, false, 1, false), F(DIF, 623, 623, false, 1, false), F(SIF, 624, 624, false, 1, false),
        F(AIF, 625, 625, false, 1, false), F(SISMAI, 626, 629, false, 1, false),
    };
    apply(f3, b, e);
    const uint64_t page = ubits(b, 615, 620);
    if (page == 1) {  // :179-212: ionosphere = bits 43:116 of the sub-frame, BDT-UTC = 117:213
        static const Field f[] = {
            F(alpha1, 657, 666, false, p2(-3), false), F(alpha2, 667, 674, true, p2(-3), false),
            F(alpha3, 675, 682, false, p2(-3), false), F(alpha4, 683, 690, false, p2(-3), false),
            F(alpha5, 691, 698, false, p2(-3), false), F(alpha6, 699, 706, true, p2(-3), false),
            F(alpha7, 707, 714, true, p2(-3), false), F(alpha8, 715, 722, true, p2(-3), false),
            F(alpha9, 723, 730, true, p2(-3), false),
            F(A_0UTC, 731, 746, true, p2(-35), false), F(A_1UTC, 747, 759, true, p2(-51), false),
            F(A_2UTC, 760, 766, true, p2(-68), false), F(delta_t_LS, 767, 774, true, 1, false),
            F(t_ot, 775, 790, false, p2(4), false), F(WN_ot, 791, 803, false, 1, false), F(WN_LSF, 804, 816, false, 1, false),
            F(DN, 817, 819, false, 1, false), F(delta_t_LSF, 820, 827, true, 1, false),
        };
        e->PageID1 = 1;
        apply(f, b, e);
    } else if (page == 3) {  // :214-229: BGTO = bits 159:226 of the sub-frame
        static const Field f[] = {
            F(GNSS_ID, 773, 775, false, 1, false), F(WN_0BGTO, 776, 788, false, 1, false),
            F(t_0BGTO, 789, 804, false, p2(4), false), F(A_0BGTO, 805, 820, true, p2(-35), false),
            F(A_1BGTO, 821, 833, true, p2(-51), false), F(A_2BGTO, 834, 840, true, p2(-68), false),
        };
        e->PageID3 = 3;
        apply(f, b, e);
    }
    if (first) e->TOW = e->HOW * 3600 + e->SOH;  // :232-234
    e->flag = 1;                                 // :237
    return 1;
}

// ---- B-CNAV2 (B2a/include/ephemeris.m), bit numbers of the 288-bit message ---------------------------------------------------
int enter_b2a(const uint8_t *b, bds_eph *e) {
    const uint64_t prn = ubits(b, 1, 6);
    if (prn < 1 || prn > 63) return 0;  // :61-64
    const int type = (int)ubits(b, 7, 12);
    e->PRN = (double)prn;
    if (std::isnan(e->SOW)) e->SOW = (double)ubits(b, 13, 30) * 3;  // isempty(eph.SOW), in every case of the switch
    // clock block of types 30..33 (:167-177 and its copies)
    static const Field clk[] = {
        F(t_oc, 43, 53, false, 300, false), F(a_0, 54, 78, true, p2(-34), false), F(a_1, 79, 100, true, p2(-50), false),
        F(a_2, 101, 111, true, p2(-66), false), F(IODC_MSB2, 112, 113, false, 1, false), F(IODC_LSB8, 114, 121, false, 1, false),
    };
    switch (type) {
    case 10: {  // :76-117
        static const Field f[] = {
            F(WN, 31, 43, false, 1, false), F(DIF, 44, 44, false, 1, false), F(SIF, 45, 45, false, 1, false),
            F(AIF, 46, 46, false, 1, false), F(t_oe, 62, 72, false, 300, false), F(deltaA, 75, 100, true, p2(-9), false),
            F(ADot, 101, 125, true, p2(-21), false), F(delta_n_0, 126, 142, true, p2(-44), true),
            F(delta_n_0Dot, 143, 165, true, p2(-57), true), F(M_0, 166, 198, true, p2(-32), true),
            F(e, 199, 231, false, p2(-34), false), F(omega, 232, 264, true, p2(-32), true),
        };
        e->idValid[0] = 10;
        apply(f, b, e);
        sat_type(ubits(b, 73, 74), e);
        break;
    }
    case 11: {  // :119-155
        static const Field f[] = {
            F(HS, 31, 32, false, 1, false), F(DIF, 33, 33, false, 1, false), F(SIF, 34, 34, false, 1, false),
            F(AIF, 36, 36, false, 1, false),  // :135 reads bit 36, not 35, as in the reference
            F(omega_0, 43, 75, true, p2(-32), true), F(i_0, 76, 108, true, p2(-32), true),
            F(omegaDot, 109, 127, true, p2(-44), true), F(i_0Dot, 128, 142, true, p2(-44), true),
            F(C_is, 143, 158, true, p2(-30), false), F(C_ic, 159, 174, true, p2(-30), false),
            F(C_rs, 175, 198, true, p2(-8), false), F(C_rc, 199, 222, true, p2(-8), false),
            F(C_us, 223, 243, true, p2(-30), false), F(C_uc, 244, 264, true, p2(-30), false),
        };
        e->idValid[1] = 11;
        apply(f, b, e);
        break;
    }
    case 30: {  // :157-187
        static const Field f[] = {
            F(alpha1, 146, 155, false, p2(-3), false), F(alpha2, 156, 163, true, p2(-3), false),
            F(alpha3, 164, 171, false, p2(-3), false), F(alpha4, 172, 179, false, p2(-3), false),
            F(alpha5, 180, 187, false, p2(-3), false), F(alpha6, 188, 195, true, p2(-3), false),
            F(alpha7, 196, 203, true, p2(-3), false), F(alpha8, 204, 211, true, p2(-3), false),
            F(alpha9, 212, 219, true, p2(-3), false),
        };
        e->idValid[2] = 30;
        apply(clk, b, e);
        apply(f, b, e);
        break;
    }
    case 31:  // :189-210
        e->idValid[3] = 31;
        apply(clk, b, e);
        break;
    case 32:  // :212-233
        e->idValid[4] = 32;
        apply(clk, b, e);
        break;
    case 33: {  // :235-264
        static const Field f[] = {
            F(GNSS_ID, 112, 114, false, 1, false),  // :258 overlaps IODC_MSB2 (112:113) and IODC_LSB8, as in the reference
            F(WN_0BGTO, 115, 127, false, 1, false), F(t_0BGTO, 128, 143, false, p2(4), false),
            F(A_0BGTO, 144, 159, true, p2(-35), false), F(A_1BGTO, 160, 172, true, p2(-51), false),
            F(A_2BGTO, 173, 179, true, p2(-68), false),
        };
        e->idValid[5] = 33;
        apply(clk, b, e);
        apply(f, b, e);
        break;
    }
    case 34: {  // :266-296
        static const Field f[] = {
            F(t_oc, 65, 75, false, 300, false), F(a_0, 76, 100, true, p2(-34), false), F(a_1, 101, 122, true, p2(-50), false),
            F(a_2, 123, 133, true, p2(-66), false), F(IODC_MSB2, 134, 135, false, 1, false),
            F(IODC_LSB8, 136, 143, false, 1, false),
            // :288-296: all nine BDT-UTC fields read bits 123:133 (a_2's), as in the reference
            F(A_0UTC, 123, 133, true, p2(-35), false), F(A_1UTC, 123, 133, true, p2(-51), false),
            F(A_2UTC, 123, 133, true, p2(-68), false), F(delta_t_LS, 123, 133, true, 1, false),
            F(t_ot, 123, 133, false, p2(4), false), F(WN_ot, 123, 133, false, 1, false), F(WN_LSF, 123, 133, false, 1, false),
            F(DN, 123, 133, false, 1, false), F(delta_t_LSF, 123, 133, true, 1, false),
        };
        e->idValid[6] = 34;
        apply(f, b, e);
        break;
    }
    default:  // :299-308
        e->idValid[7] = type;
        break;
    }
    e->flag = 1;
    return 1;
}

}  // namespace

const NavTables &nav_tables() {
    static const NavTables t = make_tables();
    return t;
}

void nav_eph_init(bds_eph *e) {
    const uint32_t size = e->size;
    *e = bds_eph{};
    e->size = size;
    const double nan = std::numeric_limits<double>::quiet_NaN();
#define BDS_EPH_X(name) e->name = nan;
    BDS_EPH_FIELDS(BDS_EPH_X)
#undef BDS_EPH_X
}

int nav_enter(int signal, const uint8_t *bits, bds_eph *e) {
    const int in = signal == BDS_SIGNAL_B1C ? enter_b1c(bits, e) : enter_b2a(bits, e);
    e->n_entered += in;
    return in;
}

}  // namespace bds

extern "C" int bds_nav_fields(int signal, const uint8_t *bits, int n_msg, int stride, bds_eph *eph) {
    if ((signal != BDS_SIGNAL_B1C && signal != BDS_SIGNAL_B2A) || n_msg < 0 || (n_msg && !bits) || !eph) return BDS_ERR_ARG;
    if (eph->size != sizeof(bds_eph)) return BDS_ERR_ARG;
    if (stride < (signal == BDS_SIGNAL_B1C ? (BDS_NAV_BITS_B1C + 7) / 8 : BDS_NAV_BITS_B2A / 8)) return BDS_ERR_ARG;
    bds::nav_eph_init(eph);
    int entered = 0;
    for (int i = 0; i < n_msg; ++i) entered += bds::nav_enter(signal, bits + (size_t)i * stride, eph);
    return entered;
}
