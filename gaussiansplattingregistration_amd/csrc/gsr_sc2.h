// gsr_sc2.h -- the layout csrc/sc2.hip agrees on with itself and with its test hooks: the tile of k_sc2_rows, the padding of the
// compatibility matrix that tile asks for, and the host arrays gsr_test_sc2_stages fills.  DESIGN.md section 33.
#pragma once
#include "gsr_common.h"

namespace gsr {

#define SC2_BM 64            // rows of A (seeds) per workgroup of k_sc2_rows: 2 waves x one 32-row MFMA tile
#define SC2_BN 128           // rows of B (correspondences) per workgroup: 2 waves x two 32-column MFMA tiles
#define SC2_BK 64            // bytes of K per LDS stage: two steps of v_mfma_i32_32x32x32_i8
#define SC2_LDS_ROW 80       // an LDS row: SC2_BK bytes and one 16-byte slot of padding (consecutive rows start 5 slots apart)
#define SC2_BLOCK 256
#define SC2_KMAX 64          // = GSR_SC2_MAX_K: the largest consensus set
#define SC2_REFINE_BLOCKS 128
#define SC2_NSTAGE 6         // timed stages: gather + compat, seed sort, rows, sets, score, refinement

inline int64_t sc2_round_up(int64_t x, int64_t to) { return (x + to - 1) / to * to; }

// Host arrays of gsr_test_sc2_stages (any may be NULL): what the stages of one call left on the device.
struct Sc2Stages {
    int32_t* deg;            // [m]
    int32_t* seeds;          // [n_seeds] correspondence of every rank
    int32_t* rows;           // [n_seeds * m] the masked second-order rows
    int32_t* k1;             // [n_seeds * 64] K1 in selection order, -1 behind its end
    int32_t* k2;             // [n_seeds * 64] K2 in selection order, -1 behind its end
    double* hyp;             // [n_seeds * 12] rows 0..2 of T_s
    int32_t* good;           // [n_seeds] inliers of T_s, -1 for an invalid seed
    double* rmse;            // [n_seeds]
    float* stage_ms;         // [SC2_NSTAGE] stream-event times of the stages (gsr_test_sc2_timed)
};

}  // namespace gsr
