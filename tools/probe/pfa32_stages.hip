// Stage driver of the N-point search pair at 53 MS/s (csrc/bds_acq_pfa32.h) for tests/test_pfa32_stages_gpu.py: reads a case file
// written by tests/pfa32_cases.py and runs the stage the case names through pfa32::Plan's forward / launch_rows / launch_cols -- the
// functions csrc/bds_acq.hip launches through, so the launch under test is the library's by construction -- and writes the raw device
// results to an output file.  The file format, the checks and the stages: tools/probe/pfa_stages_common.h.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast -fno-slp-vectorize -I bds-3-b1c-b2a-sdr-receiver_amd/csrc
//         tools/probe/pfa32_stages.hip -o pfa32_stages && ./pfa32_stages case.bin out.bin
//
//   stage 1  dst: doubled [53][32][1250] (one batch, stride 0); else nb batches `stride` apart
//   stage 2  [1] uint32 Xs[53][32][1250]
//   stats: [0] wave items, [1] output blocks whose values were compared or listed
#include "bds_acq_pfa32.h"
#include "pfa_stages_common.h"

using namespace bds::pfa32;

struct ArrayLoader {  // the forward kernels' input: x[n] of transform `batch`
    const float2 *x;
    __device__ __forceinline__ float2 operator()(int batch, long n) const { return x[(size_t)batch * NP + n]; }
};

int main(int argc, char **argv) {
    return stage_main<Plan, ArrayLoader>(argc, argv, "pfa32_stages", [](int nb, int doubled, long stride) {
        return nb >= 1 && nb <= 4 && (doubled ? nb == 1 && stride == 0 : stride >= NP && stride <= 4 * NP);
    });
}
