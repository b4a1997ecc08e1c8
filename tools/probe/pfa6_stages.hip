// Stage driver of the opt-in N-point search pair for B2a at 99.375 MS/s (csrc/bds_acq_pfa6.h) for tests/test_pfa6_stages_gpu.py: reads a
// case file written by tests/pfa6_cases.py and runs the stage the case names through pfa6::Plan's forward / launch_rows / launch_cols --
// the functions csrc/bds_acq.hip launches through, so the launch under test is the library's by construction -- and writes the raw device
// results to an output file.  The file format, the checks and the stages: tools/probe/pfa_stages_common.h; this plan's own:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast -fno-slp-vectorize -I bds-3-b1c-b2a-sdr-receiver_amd/csrc
//         tools/probe/pfa6_stages.hip -o pfa6_stages && ./pfa6_stages case.bin out.bin
//
//   stage 1  dst: nb batches `stride` apart; doubled: rows [53][6][1250], else [53][6][625]
//   stage 2  header {magic, 2, ncells, gc, p, q, nslots, guard elements, write Bw?, nspec};  [1] uint32 Xs[nspec][53][6][1250];
//            [5] double launches[n][11];  [6] int32 rng[ncells][4] or empty;  [7] int32 src[ncells] or empty
//   stage 3  [2] double launches[n][11];  [3] int32 rng[listed][4] or empty;  [4] int32 src[listed] or empty
// A column launch carries an eleventh field, masked?: a masked launch runs k_pfa6_cols<true> on its first `ncells` ranges (and sources, if
// the case has them).  stats: [0] wave items, [1] output blocks whose values were compared or listed
#include "bds_acq_pfa6.h"
#include "pfa_stages_common.h"

using namespace bds::pfa6;

struct ArrayLoader {  // the forward kernels' input: x[n] of transform `batch`
    const float2 *x;
    __device__ __forceinline__ float2 operator()(int batch, long n) const { return x[(size_t)batch * NP + n]; }
};

// the column launches on the device's inter-pass buffer of `bw_cells` cells, with the masked launches' ranges and sources
static void run_cols6(const uint32_t *d_Bw, int bw_cells, const Bytes &table, const Bytes &rng, const Bytes &src, Writer &out) {
    REQUIRE(rng.size() % 16 == 0 && src.size() % 4 == 0);
    const int nrng = (int)(rng.size() / 16), nsrc = (int)(src.size() / 4);
    REQUIRE(nsrc == 0 || nsrc == nrng);
    for (int i = 0; i < nsrc; ++i) REQUIRE(((const int *)src.data())[i] >= 0 && ((const int *)src.data())[i] < bw_cells);  // every source names a cell of the buffer
    for (int i = 0; i < 4 * nrng; ++i) REQUIRE(((const int *)rng.data())[i] >= -1 && ((const int *)rng.data())[i] < NP);
    const int4 *d_rng = upload<int4>(rng);
    const int *d_src = upload<int>(src);
    run_cols<Plan>(d_Bw, table, 11, [&](const double *p, ColsArgs &ca) {
        const bool masked = (int)p[10];
        REQUIRE(masked ? ca.ncells <= nrng && (nsrc || ca.ncells <= bw_cells) : ca.ncells <= bw_cells);
        ca.rng = masked ? d_rng : nullptr;  // (launch_cols: the masked kernel where the launch has ranges)
        ca.src = masked && nsrc ? d_src : nullptr;
    }, out);
}

int main(int argc, char **argv) {
    Case c(argc, argv, "pfa6_stages");
    if (c.stage == 1) {
        run_forward<Plan, ArrayLoader>(c, [](int nb, int doubled, long stride) {
            return nb >= 1 && nb <= kMaxQ && stride >= (doubled ? 2 * NP : NP) && stride <= 4 * NP;
        });
    } else if (c.stage == 2) {
        REQUIRE(c.nh >= 10 && c.in.size() == 8);
        const int ncells = (int)c.H[2], p = (int)c.H[4], q = (int)c.H[5], nspec = (int)c.H[9];
        REQUIRE(p >= 1 && q >= 1 && q <= kMaxQ && nspec >= q && nspec <= kMaxQ);
        const uint32_t *d_Bw = run_rows<Plan>(
            c, ncells, (int)c.H[3], (int)c.H[6], (size_t)c.H[7], (int)c.H[8], (size_t)nspec * kSpecElems * 4,
            [&](int bin) { return (long)(bin / q) * p < NP; }, [&](RowsArgs ra) { return ra.p = p, ra.q = q, ra; });
        run_cols6(d_Bw, ncells, c.in[5], c.in[6], c.in[7], c.out);
    } else if (c.stage == 3) {
        int ncells = 0;
        const uint32_t *d_Bw = upload_cells<Plan>(c, 5, &ncells);
        run_cols6(d_Bw, ncells, c.in[2], c.in[3], c.in[4], c.out);
    } else {
        REQUIRE(!"known stage");
    }
    return c.finish();
}
