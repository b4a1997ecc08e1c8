// Navigation decoding, shared between the host half (bds_nav.cpp: code tables, field parser, merging rules) and the device half
// (bds_nav.hip: the per-candidate frame decoders).
#pragma once

#include <cstdint>

#include "bds_mi355x.h"

namespace bds {

// What the host builds once and the kernels read.
struct NavTables {
    uint32_t cw21[64];   // BCH(21,6) code words, symbol 1 = bit 20 (BCH21_6Decoding.m:65-89)
    uint64_t cw51[256];  // BCH(51,8) code words, symbol 1 = bit 50 (BCH51_8Decoding.m:63-87)
    uint32_t crc[600];   // crc[e] = x^e mod g(x), g = 0x1864CFB (comm.CRCDetector([24 23 18 17 14 11 10 7 6 5 4 3 1 0]))
};
const NavTables &nav_tables();

// One candidate as the kernels leave it (bds_nav_frame without size / index).
struct NavRaw {
    uint32_t status;
    int32_t polarity, bch1_max, bch2_max;
    uint8_t bits[112];
};

void nav_eph_init(bds_eph *e);  // eph_structure_init: every field [] (NaN), counters zero; .size is kept
// ephemeris(navBitsBin, eph) on packed bits: 1 = entered, 0 = PRN field outside 1..63 (not entered: bds_mi355x.h)
int nav_enter(int signal, const uint8_t *bits, bds_eph *e);

}  // namespace bds
