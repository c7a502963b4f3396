// pgo_common.hpp -- what every stage of the pose-graph solver (pose_graph.hip) shares: the
// constants, the layout of a graph's scratch (PgoLayout, host and device), the per-graph context
// (PgoCtx) and LDS (PgoLds) the stages take, and the small helpers.
#pragma once
#include "ssf_device.hpp"
#include "ssf_internal.hpp"

#include <math.h>

namespace ssf {

constexpr int kPgoThreads = 256;
constexpr int kPgoRec = 78;                       // r[6], Ji[36], Jj[36] (row-major, whitened)
constexpr int kPgoNarrowLoops = 32;               // up to here: one lane per right-hand side
constexpr int kPgoMaxN = 6 * kPgoNarrowLoops;     // capacitance order of the narrow path
constexpr int kPgoTile = 2048;                    // edge index pairs staged in LDS (16 KiB)
constexpr int kPgoWideRows = (6 * SSF_PGO_MAX_LOOPS + kPgoThreads - 1) / kPgoThreads;   // per thread
constexpr int kPgoPanel = 8;                      // columns a sweep of the wide Cholesky updates
static_assert(kPgoMaxN + 1 <= kPgoThreads, "one lane per right-hand side");
static_assert(kPgoNarrowLoops <= SSF_PGO_MAX_LOOPS, "the narrow path is a subset");

// Where the regions of one graph's scratch start, in doubles from PgoGraph::scratch_off, and what
// the graph takes in all.  k = K, l = lcap (the host's bound on the loop count), n = 6 l:
//   LP    wide: the loop list (edge, i, j), 3 int32 a loop in 2 l doubles
//   X     the working poses, 7 k                REC   the records, 78 (E + 1) (record E: the prior)
//   D, O  the block factors, 36 k each          GR    the gradient, 6 k
//   Z     narrow: the 6 k x (n + 1) right-hand sides; wide: the 6 k x kPgoThreads pass buffer
//   CM    the capacitance matrix, n^2           VA, VB  wide: the capacitance vectors, n each
//                                               (narrow: they are in LDS, so XT follows CM)
//   XT, RECT, WS, WST  step control: the trial poses and records, and (weight, s) of every edge at
//         the accepted and at the trial point (2 E each); they follow everything else, so the
//         rest of the layout is the same with and without them
// and 8 doubles of slack.
struct PgoLayout {
    size_t LP, X, REC, D, O, GR, Z, CM, VA, VB, XT, RECT, WS, WST, total;
    __host__ __device__ constexpr PgoLayout(int K, int E, int lcap, bool wide, bool lm)
        : LP(0), X(wide ? 2 * (size_t)lcap : 0), REC(X + 7 * (size_t)K),
          D(REC + (size_t)kPgoRec * ((size_t)E + 1)), O(D + 36 * (size_t)K), GR(O + 36 * (size_t)K),
          Z(GR + 6 * (size_t)K), CM(Z + 6 * (size_t)K * (wide ? (size_t)kPgoThreads : 6 * (size_t)lcap + 1)),
          VA(CM + 36 * (size_t)lcap * (size_t)lcap), VB(VA + (wide ? 6 * (size_t)lcap : 0)),
          XT(VB + (wide ? 6 * (size_t)lcap : 0)), RECT(XT + (lm ? 7 * (size_t)K : 0)),
          WS(RECT + (lm ? (size_t)kPgoRec * ((size_t)E + 1) : 0)), WST(WS + (lm ? 2 * (size_t)E : 0)),
          total(WST + (lm ? 2 * (size_t)E : 0) + 8) {}
};

// the closed forms of DESIGN.md 6.7 (narrow and wide, each without and with step control)
constexpr bool pgo_layout_checks(size_t K, size_t E, size_t l) {
    const size_t n = 6 * l, narrow = 85 * K + 78 * (E + 1) + 6 * K * (n + 1) + n * n + 8,
                 wide = 85 * K + 78 * (E + 1) + 6 * K * kPgoThreads + n * n + 2 * n + 2 * l + 8,
                 trial = 7 * K + 78 * (E + 1) + 4 * E;
    const int k = (int)K, e = (int)E, c = (int)l;
    return PgoLayout(k, e, c, false, false).total == narrow && PgoLayout(k, e, c, true, false).total == wide &&
           PgoLayout(k, e, c, false, true).total == narrow + trial && PgoLayout(k, e, c, true, true).total == wide + trial;
}
static_assert(pgo_layout_checks(2, 1, 0) && pgo_layout_checks(5, 6, 2) && pgo_layout_checks(40, 80, 41),
              "PgoLayout::total against the formulas of DESIGN.md 6.7");

// One graph as its work-group sees it: the counts, its slices of the call's arrays, its scratch
// regions (PgoLayout) and its outputs.  Filled by pgo_prologue; uniform over the work-group
// except tid.  The stages take it by const reference and are inlined, so it lives in registers.
struct PgoCtx {
    int tid, K, E, L, n, NC, max_iter;             // L loop edges, n = 6 L, NC = n + 1 columns
    int rkind;
    double rk, func_tol;
    size_t zs;                                     // stride of a column's entries in Z
    double* P;                                     // the caller's poses: read once, written at the end
    const int32_t* IJ;
    const double *ZM, *ZV, *PP, *PV;
    int32_t* LP;
    double *X, *REC, *D, *O, *GR, *Z, *CM, *VA, *VB;
    double *XT, *RECT, *WS, *WST;                  // step control: an accepted trial swaps the pairs
    double *st, *clog, *EO, *LL;                   // stats row; nullable: cost log, edge output, lm log
};

// The work-group's LDS.  The narrow path keeps its loop list and capacitance vectors here.
struct PgoLdsCommon {
    double red[kPgoThreads / 64];
    int2 ij[kPgoTile];
    double piv;
    int bad, nloop, fail;
};
template <bool kWide>
struct PgoLds : PgoLdsCommon {};
template <>
struct PgoLds<false> : PgoLdsCommon {
    double va[kPgoMaxN], vb[kPgoMaxN];
    int loop_e[kPgoNarrowLoops], loop_i[kPgoNarrowLoops], loop_j[kPgoNarrowLoops];
};

SSF_DEV bool pgo_finite(double v) { return fabs(v) <= 1.79769313486231570e308; }   // false for NaN

SSF_DEV void pgo_quat_R(const double q[4], double R[9]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}

SSF_DEV void pgo_quat_unit(const double* q, double o[4]) {
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int k = 0; k < 4; ++k) o[k] = q[k] / n;
}

// Log of a unit quaternion as a rotation vector (theta in [0, pi])
SSF_DEV void pgo_quat_log(const double q[4], double phi[3]) {
    const double s = q[3] < 0 ? -1.0 : 1.0;
    const double x = s * q[0], y = s * q[1], z = s * q[2], w = s * q[3];
    const double n = sqrt(x * x + y * y + z * z);
    const double k = n < 1e-12 ? 2.0 / w : 2.0 * atan2(n, w) / n;
    phi[0] = k * x; phi[1] = k * y; phi[2] = k * z;
}

SSF_DEV double pgo_block_max(double v, double* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, kWave));
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane_id() == 0) lds[w] = v;
    __syncthreads();
    double m = lds[0];
    for (int i = 1; i < nw; ++i) m = fmax(m, lds[i]);
    __syncthreads();
    return m;
}

// the right-hand side of one column of [ -g | A^T ] at node k: col 0 is -g, col 1 + 6 l + row is
// row `row` of loop l's Jacobians (lrec: that loop's record), at its nodes li and lj
struct PgoColumn {
    int col, row, li, lj;
    const double* lrec;
    const double* GR;
    SSF_DEV void operator()(int k, double b[6]) const {
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            if (col == 0) b[r] = -GR[6 * (size_t)k + r];
            else if (k == li) b[r] = lrec[6 + 6 * row + r];
            else if (k == lj) b[r] = lrec[42 + 6 * row + r];
            else b[r] = 0.0;
        }
    }
};

}  // namespace ssf
