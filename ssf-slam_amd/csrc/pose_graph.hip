// pose_graph.hip -- the pose-graph optimisation of mapOptmization (runOptimize,
// src/mapOptmization.cpp:280-293, over the factors of :147-165,274) on gfx950: batched
// Gauss-Newton on SE(3), one work-group per graph, the whole iteration loop on the device.
//
//   poses        7 doubles, q(x, y, z, w) then t; tangent = (rotation, translation), GTSAM's
//                Pose3 order; retraction X (+) d = X * [Exp(w), v] (right-multiplied, first-order
//                translation: GTSAM's chart with GTSAM_POSE3_EXPMAP off).
//   factors      between (i, j, Z, var): E = Z^-1 Xi^-1 Xj, r = [Log(R_E); t_E] / sigma;
//                prior (P, var) on node 0: the same with Xi = identity, Z = P.
//   per iteration (every phase is work-group wide, separated by barriers):
//     linearise  one thread per factor: whitened residual and the two 6x6 Jacobians (78 doubles)
//     assemble   one thread per node walks the edge list (staged through LDS) in order (fixed
//                summation order, no floating-point atomics): the gradient over every factor, and the block-
//                tridiagonal part T (prior + edges with |i - j| == 1) as diagonal blocks D_k
//                and sub-diagonal blocks O_k = H[k+1][k]
//     factor     block Cholesky of T, serial over the nodes on one lane (depth K); the next
//                node's diagonal block is loaded while the current one is factored
//     substitute one lane per right-hand side: -g and the 6 L columns of A^T, A = the whitened
//                Jacobian rows of the L loop edges (every edge with |i - j| != 1); forward and
//                back substitution, serial over the nodes, the block factors read at a wave-
//                uniform address one step ahead of their use
//     Woodbury   capacitance C = I + A T^-1 A^T (6L x 6L), dense Cholesky with one thread per
//                row, dx = T^-1 b - T^-1 A^T C^-1 A T^-1 b
//     retract    one thread per node
//   The above is k_pose_graph, for graphs with at most 32 edges beyond the K - 1 of a chain
//   (so at most 32 loop edges).  Every other graph is k_pose_graph_wide's (up to
//   SSF_PGO_MAX_LOOPS loop edges); same phases, except
//     substitute the 6 L + 1 columns go through kPgoThreads at a time in a 6K x kPgoThreads pass
//                buffer; a lane folds its solved column into C (column 0 into u = A T^-1 (-g))
//                before the buffer is reused, so T^-1 A^T is never held whole
//     Woodbury   the loop list, C (order up to 1536) and its vectors live in the graph's scratch;
//                dense Cholesky with the rows strided over the threads, by panels of columns;
//                dx = T^-1 (-g - A^T w): one more single-column substitution on lane 0
//   The host picks the kernel (PgoGraph::wide, from K and E); the two share pgo_solve.
//   k_pose_graph_robust / k_pose_graph_wide_robust are the same two solvers with an m-estimator on
//   the loop edges (ssf_pgo_robust; IRLS, Triggs' first-order form): at every linearisation a loop
//   edge's record is scaled by sqrt(w(s)), s its squared whitened residual, and it enters the cost
//   with 2 rho(s).  Chain edges and the prior stay quadratic, so T is what it is without the loss.
//   They also report every edge's weight and s (d_edge_out).
//   k_pose_graph_lm / k_pose_graph_wide_lm are the loss kernels with Levenberg-Marquardt step control
//   (ssf_pgo_lm): T is damped by D / radius, the step goes to a trial point, and only a trial that
//   lowers the cost by enough of what the model promised becomes the point (see pgo_solve).
//   No inter-work-group communication of any kind.  A graph writes its poses back only when it
//   ends with SSF_PGO_OK / SSF_PGO_CONVERGED: it iterates on a copy in the context scratch.
//   Every loop bound is a count the prologue validated (K, E from the host descriptor checked
//   against the device offsets, L <= SSF_PGO_MAX_LOOPS).
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

bool pgo_graph_wide(int K, int E) { return E - (K - 1) > kPgoNarrowLoops; }

size_t pgo_graph_doubles(int K, int E, int lcap, bool wide, bool lm) {
    const size_t k = (size_t)K, nc = 6 * (size_t)lcap + 1, n = 6 * (size_t)lcap;
    const size_t head = 7 * k + (size_t)kPgoRec * ((size_t)E + 1) + 36 * k + 36 * k + 6 * k;
    // step control: the trial poses and records, and (weight, s) of every edge at both points; they
    // follow everything else, so the rest of the layout is the same with and without them
    const size_t trial = lm ? 7 * k + (size_t)kPgoRec * ((size_t)E + 1) + 4 * (size_t)E : 0;
    // wide: the loop list (3 int32 a loop), one pass buffer, C, and the two capacitance vectors
    if (wide) return head + 2 * (size_t)lcap + 6 * k * (size_t)kPgoThreads + n * n + 2 * n + trial + 8;
    return head + 6 * k * nc + n * n + trial + 8;
}

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

// the whitened residual and Jacobians of one between factor (prior: Xi = identity, Ji unused)
SSF_DEV void pgo_linearise(const double qi[4], const double ti[3], const double qj[4], const double tj[3],
                           const double* zm, const double* var, double* rec) {
    double qz[4], Ri[9], Rj[9], Rz[9];
    pgo_quat_unit(zm, qz);
    pgo_quat_R(qi, Ri); pgo_quat_R(qj, Rj); pgo_quat_R(qz, Rz);
    const double d[3] = {tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2]};
    double RM[9], tM[3], RE[9], tE[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) RM[3 * r + c] = Ri[r] * Rj[c] + Ri[3 + r] * Rj[3 + c] + Ri[6 + r] * Rj[6 + c];
        tM[r] = Ri[r] * d[0] + Ri[3 + r] * d[1] + Ri[6 + r] * d[2];
    }
    const double dz[3] = {tM[0] - zm[4], tM[1] - zm[5], tM[2] - zm[6]};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) RE[3 * r + c] = Rz[r] * RM[c] + Rz[3 + r] * RM[3 + c] + Rz[6 + r] * RM[6 + c];
        tE[r] = Rz[r] * dz[0] + Rz[3 + r] * dz[1] + Rz[6 + r] * dz[2];
    }
    const double qic[4] = {-qi[0], -qi[1], -qi[2], qi[3]}, qzc[4] = {-qz[0], -qz[1], -qz[2], qz[3]};
    double qm[4], qe[4], phi[3];
    quat_mul(qic, qj, qm);
    quat_mul(qzc, qm, qe);
    pgo_quat_unit(qe, qe);
    pgo_quat_log(qe, phi);
    // Jr^-1(phi) = I + P/2 + c P^2, P = [phi]x, P^2 = phi phi^T - theta^2 I
    const double th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2], th = sqrt(th2);
    const double cc = th < 1e-8 ? 0.0 : 1.0 / th2 - (1.0 + cos(th)) / (2.0 * th * sin(th));
    double Jr[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Jr[3 * r + c] = cc * (phi[r] * phi[c] - (r == c ? th2 : 0.0)) + (r == c ? 1.0 : 0.0);
    Jr[1] -= 0.5 * phi[2]; Jr[2] += 0.5 * phi[1];
    Jr[3] += 0.5 * phi[2]; Jr[5] -= 0.5 * phi[0];
    Jr[6] -= 0.5 * phi[1]; Jr[7] += 0.5 * phi[0];
    const double S[9] = {0.0, -tM[2], tM[1], tM[2], 0.0, -tM[0], -tM[1], tM[0], 0.0};   // [t_M]x
    double w[6];
    for (int c = 0; c < 6; ++c) w[c] = 1.0 / sqrt(var[c]);
    double* Ji = rec + 6;
    double* Jj = rec + 42;
    for (int r = 0; r < 3; ++r) {
        rec[r] = phi[r] * w[r];
        rec[3 + r] = tE[r] * w[3 + r];
        for (int c = 0; c < 3; ++c) {
            Jj[6 * r + c] = Jr[3 * r + c] * w[r];
            Jj[6 * r + 3 + c] = 0.0;
            Jj[6 * (3 + r) + c] = 0.0;
            Jj[6 * (3 + r) + 3 + c] = RE[3 * r + c] * w[3 + r];
            // -(Jr^-1 R_M^T)[r][c] = -sum_k Jr[r][k] RM[c][k]
            Ji[6 * r + c] = -(Jr[3 * r] * RM[3 * c] + Jr[3 * r + 1] * RM[3 * c + 1] + Jr[3 * r + 2] * RM[3 * c + 2]) * w[r];
            Ji[6 * r + 3 + c] = 0.0;
            // (R_Z^T [t_M]x)[r][c] = sum_k Rz[k][r] S[k][c]
            Ji[6 * (3 + r) + c] = (Rz[r] * S[c] + Rz[3 + r] * S[3 + c] + Rz[6 + r] * S[6 + c]) * w[3 + r];
            Ji[6 * (3 + r) + 3 + c] = -Rz[3 * c + r] * w[3 + r];
        }
    }
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

// The m-estimators of ssf_pgo_robust on the whitened error norm e = sqrt(s) (GTSAM's convention):
// -> (the weight w(s), 2 rho(s)), by value: an out-parameter of a function that is not inlined
// would live in scratch memory.  Out of line: the linearise phase is not the register peak.
__device__ __noinline__ double2 pgo_robust_loss(int kind, double k, double s) {
    double w = 1.0, r2 = s;
    if (kind == SSF_PGO_ROBUST_HUBER) {
        const double e = sqrt(s);
        if (e > k) { w = k / e; r2 = 2.0 * k * (e - 0.5 * k); }
    } else if (kind == SSF_PGO_ROBUST_CAUCHY) {
        const double k2 = k * k;
        w = k2 / (k2 + s);
        r2 = k2 * log1p(s / k2);
    } else if (kind == SSF_PGO_ROBUST_GEMAN_MCCLURE) {
        const double k2 = k * k, c = k2 / (k2 + s);
        w = c * c;
        r2 = c * s;
    }
    return make_double2(w, r2);
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

// T^-1 of one column on one lane: forward and back substitution through the block factors
// (D: L_k with reciprocal diagonal, O: M_k), serial over the nodes.  The column lives at
// z[(6 k + r) * zs]; the block factors are read one step ahead of their use.
SSF_DEV void pgo_substitute(const double* D, const double* O, int K, double* z, size_t zs, const PgoColumn& rhs) {
    double y[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    // Ln / Mn: the blocks of the next step (L_k and the M that couples it to the step
    // before), loaded while the current step computes
    double Ln[36], Mn[36];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            if (c <= a) Ln[6 * a + c] = D[6 * a + c];
            Mn[6 * a + c] = 0.0;
        }
    for (int k = 0; k < K; ++k) {
        double Lk[36], M[36];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                if (c <= a) Lk[6 * a + c] = Ln[6 * a + c];
                M[6 * a + c] = Mn[6 * a + c];
            }
        if (k + 1 < K) {
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    if (c <= a) Ln[6 * a + c] = D[36 * (size_t)(k + 1) + 6 * a + c];
                    Mn[6 * a + c] = O[36 * (size_t)(k) + 6 * a + c];
                }
        }
        double b[6];
        rhs(k, b);
        if (k > 0) {
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) b[r] -= M[6 * r + c] * y[c];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double s = b[r];
#pragma unroll
            for (int c = 0; c < r; ++c) s -= Lk[6 * r + c] * y[c];
            y[r] = s * Lk[6 * r + r];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) z[(6 * (size_t)k + r) * zs] = y[r];
    }
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double bn[6];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            if (c <= a) Ln[6 * a + c] = D[36 * (size_t)(K - 1) + 6 * a + c];
            Mn[6 * a + c] = 0.0;
        }
#pragma unroll
    for (int r = 0; r < 6; ++r) bn[r] = z[(6 * (size_t)(K - 1) + r) * zs];
    for (int k = K - 1; k >= 0; --k) {
        double Lk[36], M[36];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                if (c <= a) Lk[6 * a + c] = Ln[6 * a + c];
                M[6 * a + c] = Mn[6 * a + c];
            }
        double b[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) b[r] = bn[r];
        if (k > 0) {
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    if (c <= a) Ln[6 * a + c] = D[36 * (size_t)(k - 1) + 6 * a + c];
                    Mn[6 * a + c] = O[36 * (size_t)(k - 1) + 6 * a + c];
                }
#pragma unroll
            for (int r = 0; r < 6; ++r) bn[r] = z[(6 * (size_t)(k - 1) + r) * zs];
        }
        if (k + 1 < K) {
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) b[r] -= M[6 * c + r] * x[c];
        }
#pragma unroll
        for (int r = 5; r >= 0; --r) {
            double s = b[r];
#pragma unroll
            for (int c = r + 1; c < 6; ++c) s -= Lk[6 * c + r] * x[c];
            x[r] = s * Lk[6 * r + r];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) z[(6 * (size_t)k + r) * zs] = x[r];
    }
}

// The solver of both kernels.  kWide = false: up to kPgoNarrowLoops loop edges, every right-hand
// side on a lane of its own, the loop list and the capacitance vectors in LDS.  kWide = true: up
// to SSF_PGO_MAX_LOOPS, the columns of A^T in passes of kPgoThreads, everything sized by L in the
// graph's scratch.  A work-group whose graph belongs to the other kernel returns at once.
// kRobust: the loss (rkind, rk) on the loop edges, and edge_out (nullable): two doubles per edge
// (SSF_PGO_EDGE_*) at the host's edge offsets, NaN for a graph that fails.
// kLM: Levenberg-Marquardt step control (ssf_pgo_lm; Ceres' LevenbergMarquardtStrategy, as k_solve's).
// One pass of the loop is then one attempt: T gets D / radius on its diagonal (D: the clamped
// diagonal of the full J^T J), the step goes to a trial copy of the poses, and the next pass
// linearises the trial point and accepts it (the two pose and record buffers swap) or rejects it.
// lm_log (nullable): SSF_PGO_LM_LOG_STRIDE doubles per attempt, NaN for a graph that fails.
template <bool kWide, bool kRobust, bool kLM = false>
SSF_DEV void pgo_solve(
    const PgoGraph* __restrict__ desc, double* __restrict__ pose, const int32_t* __restrict__ node_off,
    const int32_t* __restrict__ edge_ij, const double* __restrict__ edge_meas,
    const double* __restrict__ edge_var, const int32_t* __restrict__ edge_off,
    const double* __restrict__ prior_pose, const double* __restrict__ prior_var, int max_iter,
    double func_tol, double* scratch, double* __restrict__ stats, double* __restrict__ cost_log,
    int rkind = 0, double rk = 0.0, double* __restrict__ edge_out = nullptr, ssf_pgo_lm lm = ssf_pgo_lm{},
    double* __restrict__ lm_log = nullptr) {
    __shared__ double red[kPgoThreads / 64];
    __shared__ double va[kWide ? 1 : kPgoMaxN], vb[kWide ? 1 : kPgoMaxN];
    __shared__ int2 ij_s[kPgoTile];
    __shared__ double piv_s;
    __shared__ int bad_s, nloop_s, fail_s;
    __shared__ int loop_e[kPgoNarrowLoops], loop_i[kPgoNarrowLoops], loop_j[kPgoNarrowLoops];

    const int g = blockIdx.x, tid = threadIdx.x;
    const PgoGraph G = desc[g];
    if ((G.wide != 0) != kWide) return;
    const int K = G.K, E = G.E;
    // wide: the loop list (edge, i, j) leads the graph's scratch
    int32_t* LP = reinterpret_cast<int32_t*>(scratch + G.scratch_off);
    const int lmax = kWide ? G.lcap : kPgoNarrowLoops;
    double* st = stats + (size_t)g * SSF_PGO_OUT_STRIDE;
    double* clog = cost_log ? cost_log + (size_t)g * (size_t)(max_iter + 1) : nullptr;
    const double kNaN = __builtin_nan("");
    // the host validated its edge offsets against each other: the call's output has E rows from edge0
    double* EO = kRobust && edge_out ? edge_out + (size_t)SSF_PGO_EDGE_OUT_STRIDE * (size_t)G.edge0 : nullptr;
    double* LL = kLM && lm_log ? lm_log + (size_t)g * (size_t)max_iter * SSF_PGO_LM_LOG_STRIDE : nullptr;

    // ---- prologue: validation before any indexed access
    if (tid == 0) { bad_s = 0; nloop_s = 0; fail_s = 0; }
    __syncthreads();
    if (clog)
        for (int k = tid; k <= max_iter; k += kPgoThreads) clog[k] = kNaN;
    if constexpr (kLM)
        if (LL)
            for (int k = tid; k < SSF_PGO_LM_LOG_STRIDE * max_iter; k += kPgoThreads) LL[k] = kNaN;
    int status = -1;
    if (K == 0) status = SSF_PGO_EMPTY;
    if (node_off[g] != G.node0 || node_off[g + 1] != G.node0 + K || edge_off[g] != G.edge0 ||
        edge_off[g + 1] != G.edge0 + E)
        status = SSF_PGO_BAD_INPUT;              // the device offsets disagree with the host's
    double* P = pose + 7 * (size_t)G.node0;
    const int32_t* IJ = edge_ij + 2 * (size_t)G.edge0;
    const double* ZM = edge_meas + 7 * (size_t)G.edge0;
    const double* ZV = edge_var + 6 * (size_t)G.edge0;
    const double* PP = prior_pose + 7 * (size_t)g;
    const double* PV = prior_var + 6 * (size_t)g;
    if (status < 0) {
        int bad = 0;
        for (int k = tid; k < K; k += kPgoThreads) {
            const double* p = P + 7 * (size_t)k;
            for (int c = 0; c < 7; ++c) bad |= !pgo_finite(p[c]);
            bad |= !(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3] > 0.0);
        }
        for (int e = tid; e < E; e += kPgoThreads) {
            const int i = IJ[2 * e], j = IJ[2 * e + 1];
            bad |= (i < 0 || i >= K || j < 0 || j >= K || i == j);
            const double* z = ZM + 7 * (size_t)e;
            for (int c = 0; c < 7; ++c) bad |= !pgo_finite(z[c]);
            bad |= !(z[0] * z[0] + z[1] * z[1] + z[2] * z[2] + z[3] * z[3] > 0.0);
            for (int c = 0; c < 6; ++c) bad |= !(pgo_finite(ZV[6 * (size_t)e + c]) && ZV[6 * (size_t)e + c] > 0.0);
        }
        if (tid < 7) bad |= !pgo_finite(PP[tid]);
        if (tid == 7) bad |= !(PP[0] * PP[0] + PP[1] * PP[1] + PP[2] * PP[2] + PP[3] * PP[3] > 0.0);
        if (tid >= 8 && tid < 14) bad |= !(pgo_finite(PV[tid - 8]) && PV[tid - 8] > 0.0);
        if (bad) atomicOr(&bad_s, 1);
        __syncthreads();
        if (bad_s) status = SSF_PGO_BAD_INPUT;
    }
    int L = 0;
    if (status < 0) {
        // the loop edges in edge order (wave 0, ballot compaction)
        if (tid < kWave) {
            int cnt = 0;
            for (int b = 0; b < E; b += kWave) {
                const int e = b + tid;
                int i = 0, j = 1;
                if (e < E) { i = IJ[2 * e]; j = IJ[2 * e + 1]; }
                const bool lp = e < E && i - j != 1 && j - i != 1;
                const uint64_t m = __ballot(lp);
                const int pos = cnt + __popcll(m & lanemask_lt());
                if (lp && pos < lmax) {
                    if constexpr (kWide) { LP[3 * pos] = e; LP[3 * pos + 1] = i; LP[3 * pos + 2] = j; }
                    else { loop_e[pos] = e; loop_i[pos] = i; loop_j[pos] = j; }
                }
                cnt += __popcll(m);
            }
            if (tid == 0) nloop_s = cnt;
        }
        __syncthreads();
        L = nloop_s;
        if (L > SSF_PGO_MAX_LOOPS) status = SSF_PGO_TOO_MANY_LOOPS;
        // fewer than K - 1 chain edges: some (k, k + 1) pair is unlinked and T is singular
        else if (L > G.lcap) status = SSF_PGO_NOT_PD;
    }
    if (status >= 0) {
        if (tid == 0) {
            st[SSF_PGO_OUT_STATUS] = status; st[SSF_PGO_OUT_ITERATIONS] = 0.0;
            st[SSF_PGO_OUT_COST0] = kNaN; st[SSF_PGO_OUT_COST] = kNaN;
            st[SSF_PGO_OUT_DX] = 0.0; st[SSF_PGO_OUT_LOOPS] = status == SSF_PGO_EMPTY || status == SSF_PGO_BAD_INPUT ? 0.0 : (double)nloop_s;
            st[6] = 0.0; st[7] = 0.0;
        }
        if constexpr (kRobust)
            if (EO)
                for (int e = tid; e < SSF_PGO_EDGE_OUT_STRIDE * E; e += kPgoThreads) EO[e] = kNaN;
        return;
    }

    // ---- scratch of this graph
    const int NC = 6 * L + 1, n = 6 * L;
    double* X = scratch + G.scratch_off + (kWide ? 2 * (size_t)G.lcap : 0);
    double* REC = X + 7 * (size_t)K;
    double* D = REC + (size_t)kPgoRec * ((size_t)E + 1);
    double* O = D + 36 * (size_t)K;
    double* GR = O + 36 * (size_t)K;
    double* Z = GR + 6 * (size_t)K;
    double* CM = Z + 6 * (size_t)K * (size_t)(kWide ? kPgoThreads : 6 * G.lcap + 1);
    double* VA = CM + 36 * (size_t)G.lcap * (size_t)G.lcap;      // wide: u, then w
    double* VB = VA + 6 * (size_t)G.lcap;
    const size_t zs = kWide ? (size_t)kPgoThreads : (size_t)NC;  // stride of a column's entries in Z
    // step control: the trial point XT and its records RECT, and (weight, s) of every edge at the
    // accepted point (WS) and at the trial point (WST); an accepted trial swaps the pairs
    double* XT = kWide ? VB + 6 * (size_t)G.lcap : VA;
    double* RECT = XT + 7 * (size_t)K;
    double* WS = RECT + (size_t)kPgoRec * ((size_t)E + 1);
    double* WST = WS + 2 * (size_t)E;
    for (int k = tid; k < K; k += kPgoThreads) {
        double q[4];
        pgo_quat_unit(P + 7 * (size_t)k, q);
        for (int c = 0; c < 4; ++c) X[7 * (size_t)k + c] = q[c];
        for (int c = 4; c < 7; ++c) X[7 * (size_t)k + c] = P[7 * (size_t)k + c];
    }
    __syncthreads();

    int iters = 0;
    double cost0 = 0.0, cost = 0.0, prev = 0.0, dxmax = 0.0;
    status = SSF_PGO_OK;
    // step control, uniform over the work-group: the trust-region radius and the factor the next
    // rejection divides it by, the run of invalid steps, the accepted steps, whether XT holds a
    // trial point that waits for its evaluation, that step's model decrease and max-norm
    double radius = lm.radius0, dec = 2.0, mcc = 0.0, dxt = 0.0;
    int invalid = 0, accepted = 0;
    bool trial = false;
    // an attempt without a usable step (a pivot of the damped system failed, a non-finite step,
    // no model decrease): the radius shrinks, the point stays -> true after more than 5 in a row
    // (the body is discarded without kLM, so that it captures nothing there: a captured `cost` or
    // `iters` changes the register allocation of the kernels without step control)
    auto lm_invalid = [&](int it, double m) {
        if constexpr (!kLM) {
            return false;
        } else {
            radius /= dec;
            dec *= 2.0;
            trial = false;
            iters = it + 1;
            if (tid == 0) {
                if (clog) clog[it + 1] = cost;
                if (LL) {
                    double* ll = LL + (size_t)SSF_PGO_LM_LOG_STRIDE * it;
                    ll[SSF_PGO_LM_LOG_MCC] = m; ll[SSF_PGO_LM_LOG_RADIUS] = radius;
                    ll[SSF_PGO_LM_LOG_OUTCOME] = SSF_PGO_LM_INVALID;
                }
            }
            return ++invalid > 5;
        }
    };
    for (int it = 0; it <= max_iter; ++it) {
        // -- linearise: factor E is the prior.  Step control: pass 0 linearises the start, a later
        //    pass the trial point of the attempt before it (none after an invalid attempt)
        double* Xl = X;
        double* Rl = REC;
        double* Wl = WS;
        bool lin = true;
        if constexpr (kLM) {
            if (it > 0) { Xl = XT; Rl = RECT; Wl = WST; }
            lin = it == 0 || trial;
        }
        double cs[1] = {0.0};
        for (int e = lin ? tid : E + 1; e <= E; e += kPgoThreads) {
            double* rec = Rl + (size_t)kPgoRec * e;
            if (e < E) {
                const double* xi = Xl + 7 * (size_t)IJ[2 * e];
                const double* xj = Xl + 7 * (size_t)IJ[2 * e + 1];
                pgo_linearise(xi, xi + 4, xj, xj + 4, ZM + 7 * (size_t)e, ZV + 6 * (size_t)e, rec);
            } else {
                const double qi[4] = {0.0, 0.0, 0.0, 1.0}, ti[3] = {0.0, 0.0, 0.0};
                pgo_linearise(qi, ti, Xl, Xl + 4, PP, PV, rec);
            }
            double s = 0.0;
            for (int c = 0; c < 6; ++c) s += rec[c] * rec[c];
            if constexpr (kRobust) {
                // a loop edge: weight and 2 rho from s, its record scaled in place (what the
                // assemble phase, PgoColumn and the capacitance read)
                double w = 1.0, rho2 = s;
                if (e < E) {
                    const int i = IJ[2 * e], j = IJ[2 * e + 1];
                    if (i - j != 1 && j - i != 1) {
                        const double2 wr = pgo_robust_loss(rkind, rk, s);
                        w = wr.x;
                        rho2 = wr.y;
                        const double sw = sqrt(w);
                        for (int c = 0; c < kPgoRec; ++c) rec[c] *= sw;
                    }
                    if constexpr (kLM) {               // edge_out gets the accepted point's at the end
                        Wl[SSF_PGO_EDGE_OUT_STRIDE * (size_t)e + SSF_PGO_EDGE_WEIGHT] = w;
                        Wl[SSF_PGO_EDGE_OUT_STRIDE * (size_t)e + SSF_PGO_EDGE_CHI2] = s;
                    } else if (EO) {
                        EO[SSF_PGO_EDGE_OUT_STRIDE * (size_t)e + SSF_PGO_EDGE_WEIGHT] = w;
                        EO[SSF_PGO_EDGE_OUT_STRIDE * (size_t)e + SSF_PGO_EDGE_CHI2] = s;
                    }
                }
                cs[0] += rho2;
            } else {
                cs[0] += s;
            }
        }
        block_sum<1>(cs, red);                     // its barriers also publish REC
        if constexpr (!kLM) {
            cost = 0.5 * cs[0];
            if (tid == 0 && clog) clog[it] = cost;
            if (it == 0) cost0 = cost;
            if (it == max_iter) break;                 // the evaluation after the last retraction
            if (it > 0 && func_tol > 0.0 && fabs(prev - cost) <= func_tol * prev) { status = SSF_PGO_CONVERGED; break; }
            prev = cost;
        } else {
            if (it == 0) {
                cost = cost0 = 0.5 * cs[0];
                if (tid == 0 && clog) clog[0] = cost;
            } else if (trial) {
                // -- attempt `it` ends: accept the trial point when the cost fell by more than
                //    min_relative_decrease of what the model promised (a NaN trial cost rejects)
                const double ct = 0.5 * cs[0], rho = (cost - ct) / mcc;
                const bool acc = rho > lm.min_relative_decrease;
                bool stop = false;
                if (acc) {
                    prev = cost;
                    cost = ct;
                    double* sw = X; X = XT; XT = sw;
                    sw = REC; REC = RECT; RECT = sw;
                    sw = WS; WS = WST; WST = sw;
                    ++accepted;
                    dxmax = dxt;
                    const double t = 2.0 * rho - 1.0;
                    radius = fmin(radius / fmax(1.0 / 3.0, 1.0 - t * t * t), lm.max_radius);
                    dec = 2.0;
                    if (func_tol > 0.0 && prev - cost <= func_tol * prev) { status = SSF_PGO_CONVERGED; stop = true; }
                } else {
                    radius /= dec;
                    dec *= 2.0;
                }
                trial = false;
                if (tid == 0) {
                    if (clog) clog[it] = cost;
                    if (LL) {
                        double* ll = LL + (size_t)SSF_PGO_LM_LOG_STRIDE * (it - 1);
                        ll[SSF_PGO_LM_LOG_COST] = ct; ll[SSF_PGO_LM_LOG_MCC] = mcc;
                        ll[SSF_PGO_LM_LOG_RADIUS] = radius;
                        ll[SSF_PGO_LM_LOG_OUTCOME] = acc ? SSF_PGO_LM_ACCEPTED : SSF_PGO_LM_REJECTED;
                    }
                }
                if (stop || radius < lm.min_radius) break;
            }
            if (it == max_iter) break;
        }

        // -- assemble T (D, O) and the gradient, one thread per node, edges in order; the edge
        //    index pairs are staged through LDS in tiles, so the scan reads no global memory
        for (int kb = 0; kb < K; kb += kPgoThreads) {                      // uniform
            const int k = kb + tid;
            const bool act = k < K;
            double Dk[36], Ok[36], gk[6];
            for (int c = 0; c < 36; ++c) { Dk[c] = 0.0; Ok[c] = 0.0; }
            for (int c = 0; c < 6; ++c) gk[c] = 0.0;
            double hd[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // step control: the loop rows' part of diag(J^T J)
            bool linked = false;
            auto add = [&](int e, int i, int j) {      // factor e touches node k (e < 0: the prior)
                const double* rec = REC + (size_t)kPgoRec * (e < 0 ? E : e);
                const double* Jk = rec + (i == k ? 6 : 42);
                const bool chain = e < 0 || i - j == 1 || j - i == 1;
                const int other = i == k ? j : i;
                const bool next = e >= 0 && chain && other == k + 1;
                const double* Jo = rec + (i == k ? 42 : 6);
                linked = linked || next;
                // one Jacobian row at a time: rank-1 updates of g, D (lower) and O
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    double jk[6];
#pragma unroll
                    for (int a = 0; a < 6; ++a) jk[a] = Jk[6 * c + a];
                    const double rc = rec[c];
#pragma unroll
                    for (int a = 0; a < 6; ++a) gk[a] += jk[a] * rc;
                    if (chain) {
#pragma unroll
                        for (int a = 0; a < 6; ++a)
#pragma unroll
                            for (int b = 0; b <= a; ++b) Dk[6 * a + b] += jk[a] * jk[b];
                    }
                    if constexpr (kLM) {
                        if (!chain) {
#pragma unroll
                            for (int a = 0; a < 6; ++a) hd[a] += jk[a] * jk[a];
                        }
                    }
                    if (next) {
#pragma unroll
                        for (int a = 0; a < 6; ++a) {
                            const double jo = Jo[6 * c + a];
#pragma unroll
                            for (int b = 0; b < 6; ++b) Ok[6 * a + b] += jo * jk[b];
                        }
                    }
                }
            };
            if (k == 0) add(-1, -2, 0);                // the prior: the dj form on node 0
            for (int e0 = 0; e0 < E; e0 += kPgoTile) {                     // uniform
                const int tn = min(kPgoTile, E - e0);
                __syncthreads();
                for (int t = tid; t < tn; t += kPgoThreads)
                    ij_s[t] = make_int2(IJ[2 * (e0 + t)], IJ[2 * (e0 + t) + 1]);
                __syncthreads();
                if (act)
                    for (int t = 0; t < tn; ++t) {
                        const int2 ij = ij_s[t];
                        if (ij.x == k || ij.y == k) add(e0 + t, ij.x, ij.y);
                    }
            }
            if constexpr (kLM) {
                // H + D / radius, D = the diagonal of the full J^T J (chain edges, prior and the scaled
                // loop rows) clamped to [1e-6, 1e32]: it lands on T, the Woodbury form stays
#pragma unroll
                for (int a = 0; a < 6; ++a) Dk[7 * a] += fmin(fmax(Dk[7 * a] + hd[a], 1e-6), 1e32) / radius;
            }
            if (act) {
                for (int c = 0; c < 36; ++c) { D[36 * (size_t)k + c] = Dk[c]; O[36 * (size_t)k + c] = Ok[c]; }
                for (int c = 0; c < 6; ++c) GR[6 * (size_t)k + c] = gk[c];
                // a chain link without an edge: T is singular (in exact arithmetic; rounding
                // could let its Cholesky pass), whatever the loop edges connect
                if (k + 1 < K && !linked) atomicOr(&fail_s, 1);
            }
        }
        __syncthreads();

        // -- block Cholesky of T on one lane: D_k <- L_k (lower, reciprocal diagonal),
        //    O_k <- M_k = O_k L_k^-T
        if (tid == 0) {
            double M[36], Dn[36];                      // Dn: the next node's diagonal block, loaded ahead
            int ok = 1;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b) Dn[6 * a + b] = D[6 * a + b];
            for (int k = 0; k < K && ok; ++k) {
                double Sm[36], Oc[36];                 // Oc is used last: its load hides behind the factor
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = 0; b < 6; ++b) {
                        if (b <= a) Sm[6 * a + b] = Dn[6 * a + b];
                        Oc[6 * a + b] = O[36 * (size_t)k + 6 * a + b];
                    }
                if (k + 1 < K) {
#pragma unroll
                    for (int a = 0; a < 6; ++a)
#pragma unroll
                        for (int b = 0; b <= a; ++b) Dn[6 * a + b] = D[36 * (size_t)(k + 1) + 6 * a + b];
                }
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = 0; b <= a; ++b) {
                        double s = Sm[6 * a + b];
                        if (k > 0)
#pragma unroll
                            for (int c = 0; c < 6; ++c) s -= M[6 * a + c] * M[6 * b + c];
                        Sm[6 * a + b] = s;
                    }
#pragma unroll
                for (int b = 0; b < 6; ++b) {
                    double p = Sm[6 * b + b];
#pragma unroll
                    for (int c = 0; c < b; ++c) p -= Sm[6 * b + c] * Sm[6 * b + c];
                    if (!(p > 0.0) || !pgo_finite(p)) { ok = 0; break; }
                    const double inv = 1.0 / sqrt(p);
#pragma unroll
                    for (int a = b + 1; a < 6; ++a) {
                        double s = Sm[6 * a + b];
#pragma unroll
                        for (int c = 0; c < b; ++c) s -= Sm[6 * a + c] * Sm[6 * b + c];
                        Sm[6 * a + b] = s * inv;
                    }
                    Sm[6 * b + b] = inv;
                }
                if (!ok) break;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = 0; b <= a; ++b) D[36 * (size_t)k + 6 * a + b] = Sm[6 * a + b];
                if (k + 1 < K) {
#pragma unroll
                    for (int a = 0; a < 6; ++a)
#pragma unroll
                        for (int b = 0; b < 6; ++b) {
                            double s = Oc[6 * a + b];
#pragma unroll
                            for (int c = 0; c < b; ++c) s -= M[6 * a + c] * Sm[6 * b + c];
                            M[6 * a + b] = s * Sm[6 * b + b];
                        }
#pragma unroll
                    for (int c = 0; c < 36; ++c) O[36 * (size_t)k + c] = M[c];
                }
            }
            if constexpr (kLM) {
                if (!ok) fail_s |= 2;                  // bit 0 stays the missing chain link's
            } else {
                if (!ok) fail_s = 1;
            }
        }
        __syncthreads();
        if constexpr (kLM) {
            // a missing chain link ends the graph as without step control (damping would make
            // that singular T factorable); a failed pivot of the damped T is an invalid step
            const int f = fail_s;
            if (f & 1) { status = SSF_PGO_NOT_PD; break; }
            if (f) {
                __syncthreads();
                if (tid == 0) fail_s = 0;
                __syncthreads();
                if (lm_invalid(it, kNaN)) break;
                continue;
            }
        } else {
            if (fail_s) { status = SSF_PGO_NOT_PD; break; }
        }

        double mx = 0.0;
        if constexpr (!kWide) {
            // -- T^-1 [ -g | A^T ]: one lane per column, serial over the nodes
            if (tid < NC) {
                const int col = tid, l = col > 0 ? (col - 1) / 6 : 0, row = col > 0 ? (col - 1) % 6 : 0;
                const int li = col > 0 ? loop_i[l] : -1, lj = col > 0 ? loop_j[l] : -1;
                const double* lrec = REC + (size_t)kPgoRec * (col > 0 ? loop_e[l] : 0);
                pgo_substitute(D, O, K, Z + col, zs, PgoColumn{col, row, li, lj, lrec, GR});
            }
            __syncthreads();

            // -- Woodbury: C = I + A Z_A (column-major in CM), u = A z0, C w = u
            if (L > 0) {
                if (tid < n) {
                    const int l = tid / 6, row = tid % 6;
                    const double* lrec = REC + (size_t)kPgoRec * loop_e[l];
                    const double* zi = Z + 6 * (size_t)loop_i[l] * NC;
                    const double* zj = Z + 6 * (size_t)loop_j[l] * NC;
                    for (int b = 0; b <= n; ++b) {                 // b == 0: u; b >= 1: column b - 1
                        double s = 0.0;
                        for (int q = 0; q < 6; ++q)
                            s += lrec[6 + 6 * row + q] * zi[(size_t)q * NC + b] + lrec[42 + 6 * row + q] * zj[(size_t)q * NC + b];
                        if (b == 0) va[tid] = s;
                        else CM[(size_t)(b - 1) * n + tid] = s + (b - 1 == tid ? 1.0 : 0.0);
                    }
                }
                __syncthreads();
                for (int j = 0; j < n; ++j) {                      // Cholesky, one thread per row
                    double s = 0.0;
                    if (tid < n && tid >= j) {
                        s = CM[(size_t)j * n + tid];
                        for (int p = 0; p < j; ++p) s -= CM[(size_t)p * n + tid] * CM[(size_t)p * n + j];
                        if (tid == j) piv_s = s;
                    }
                    __syncthreads();
                    const double piv = piv_s;
                    if (!(piv > 0.0) || !pgo_finite(piv)) { status = SSF_PGO_NOT_PD; break; }   // uniform
                    if (tid < n && tid >= j) CM[(size_t)j * n + tid] = tid == j ? sqrt(piv) : s / sqrt(piv);
                    __syncthreads();
                }
                if (status == SSF_PGO_NOT_PD) {
                    if constexpr (kLM) {                           // a failed pivot of C: an invalid step
                        status = SSF_PGO_OK;
                        if (lm_invalid(it, kNaN)) break;
                        continue;
                    }
                    break;
                }
                for (int j = 0; j < n; ++j) {                      // forward: va -> vb
                    __syncthreads();
                    const double yj = va[j] / CM[(size_t)j * n + j];
                    if (tid == j) vb[j] = yj;
                    if (tid < n && tid > j) va[tid] -= CM[(size_t)j * n + tid] * yj;
                }
                for (int j = n - 1; j >= 0; --j) {                 // backward: vb -> va
                    __syncthreads();
                    const double xj = vb[j] / CM[(size_t)j * n + j];
                    if (tid == j) va[j] = xj;
                    if (tid < j) vb[tid] -= CM[(size_t)tid * n + j] * xj;
                }
                __syncthreads();
            }

            // -- dx = z0 - Z_A w (into column 0), its max-norm, then the retraction
            for (int k = tid; k < K; k += kPgoThreads)
                for (int r = 0; r < 6; ++r) {
                    double* zr = Z + (6 * (size_t)k + r) * NC;
                    double s = zr[0];
                    for (int b = 0; b < n; ++b) s -= zr[1 + b] * va[b];
                    zr[0] = s;
                    mx = pgo_finite(s) ? fmax(mx, fabs(s)) : __builtin_inf();
                }
        } else {
            // -- T^-1 [ -g | A^T ], kPgoThreads columns a pass, one lane per column.  A lane folds its
            //    solved column into the capacitance matrix (column 0, z0 = T^-1 (-g), into u = A z0)
            //    before the pass buffer is reused: T^-1 A^T is never held whole.  C = I + A Z_A is
            //    column-major in CM.  A lane reads back only what it wrote itself: no barrier in here.
            for (int c0 = 0; c0 < NC; c0 += kPgoThreads) {
                const int col = c0 + tid;
                if (col < NC) {
                    const int l = col > 0 ? (col - 1) / 6 : 0, row = col > 0 ? (col - 1) % 6 : 0;
                    const int li = col > 0 ? LP[3 * l + 1] : -1, lj = col > 0 ? LP[3 * l + 2] : -1;
                    const double* lrec = REC + (size_t)kPgoRec * (col > 0 ? LP[3 * l] : 0);
                    double* z = Z + tid;
                    pgo_substitute(D, O, K, z, zs, PgoColumn{col, row, li, lj, lrec, GR});
                    for (int m = 0; m < L; ++m) {                  // rows 6 m .. 6 m + 5 of A z
                        const double* mrec = REC + (size_t)kPgoRec * LP[3 * m];
                        const double* zi = z + 6 * (size_t)LP[3 * m + 1] * zs;
                        const double* zj = z + 6 * (size_t)LP[3 * m + 2] * zs;
                        double vi[6], vj[6];
                        for (int q = 0; q < 6; ++q) { vi[q] = zi[(size_t)q * zs]; vj[q] = zj[(size_t)q * zs]; }
                        for (int r = 0; r < 6; ++r) {
                            double s = 0.0;
                            for (int q = 0; q < 6; ++q) s += mrec[6 + 6 * r + q] * vi[q] + mrec[42 + 6 * r + q] * vj[q];
                            if (col == 0) VA[6 * m + r] = s;
                            else CM[(size_t)(col - 1) * n + 6 * m + r] = s + (col - 1 == 6 * m + r ? 1.0 : 0.0);
                        }
                    }
                }
            }
            __syncthreads();

            // -- Woodbury: C w = u by dense Cholesky, the rows strided over the threads (row
            //    tid + q kPgoThreads in slot q), then dx = T^-1 (-g - A^T w).  Left-looking by
            //    panels of kPgoPanel columns: a sweep over the columns left of the panel updates the
            //    whole panel, so C is read n / kPgoPanel times, not n times.  A slot takes part while
            //    any of its rows does (a uniform test); its rows above the diagonal read a clamped
            //    address and their sums are never stored.
            if (L > 0) {
                for (int j0 = 0; j0 < n; j0 += kPgoPanel) {
                    // t: the thread index made opaque, so that the row offsets below are not hoisted out
                    // of the iteration loop into registers the substitution phases need
                    int t = tid;
                    asm volatile("" : "+v"(t));
                    double acc[kPgoWideRows][kPgoPanel];
#pragma unroll
                    for (int q = 0; q < kPgoWideRows; ++q)
#pragma unroll
                        for (int b = 0; b < kPgoPanel; ++b) {
                            const int r = t + q * kPgoThreads;
                            acc[q][b] = r < n && r >= j0 && j0 + b < n ? CM[(size_t)(j0 + b) * n + r] : 0.0;
                        }
                    for (int p = 0; p < j0; ++p) {
                        double cj[kPgoPanel];
#pragma unroll
                        for (int b = 0; b < kPgoPanel; ++b) cj[b] = CM[(size_t)p * n + min(j0 + b, n - 1)];
#pragma unroll
                        for (int q = 0; q < kPgoWideRows; ++q)
                            if (q * kPgoThreads < n && (q + 1) * kPgoThreads > j0) {
                                const double cr = CM[(size_t)p * n + min(t + q * kPgoThreads, n - 1)];
#pragma unroll
                                for (int b = 0; b < kPgoPanel; ++b) acc[q][b] -= cr * cj[b];
                            }
                    }
#pragma unroll
                    for (int b = 0; b < kPgoPanel; ++b) {          // the panel's own columns in turn
                        const int j = j0 + b;
                        if (j >= n) break;
#pragma unroll
                        for (int c = 0; c < b; ++c) {
                            const double cjc = CM[(size_t)(j0 + c) * n + j];
#pragma unroll
                            for (int q = 0; q < kPgoWideRows; ++q) acc[q][b] -= acc[q][c] * cjc;
                        }
#pragma unroll
                        for (int q = 0; q < kPgoWideRows; ++q)
                            if (t + q * kPgoThreads == j) piv_s = acc[q][b];
                        __syncthreads();
                        const double piv = piv_s;
                        if (!(piv > 0.0) || !pgo_finite(piv)) { status = SSF_PGO_NOT_PD; break; }   // uniform
#pragma unroll
                        for (int q = 0; q < kPgoWideRows; ++q) {
                            const int r = t + q * kPgoThreads;
                            acc[q][b] = r == j ? sqrt(piv) : acc[q][b] / sqrt(piv);
                            if (r < n && r >= j) CM[(size_t)j * n + r] = acc[q][b];
                        }
                        __syncthreads();
                    }
                    if (status == SSF_PGO_NOT_PD) break;
                }
                if (status == SSF_PGO_NOT_PD) {
                    if constexpr (kLM) {
                        status = SSF_PGO_OK;
                        if (lm_invalid(it, kNaN)) break;
                        continue;
                    }
                    break;
                }
                for (int j = 0; j < n; ++j) {                      // forward: VA -> VB
                    __syncthreads();
                    const double yj = VA[j] / CM[(size_t)j * n + j];
                    if (tid == j % kPgoThreads) VB[j] = yj;
                    for (int r = tid; r < n; r += kPgoThreads)
                        if (r > j) VA[r] -= CM[(size_t)j * n + r] * yj;
                }
                for (int j = n - 1; j >= 0; --j) {                 // backward: VB -> VA
                    __syncthreads();
                    const double xj = VB[j] / CM[(size_t)j * n + j];
                    if (tid == j % kPgoThreads) VA[j] = xj;
                    for (int r = tid; r < j; r += kPgoThreads) VB[r] -= CM[(size_t)r * n + j] * xj;
                }
                __syncthreads();
                // g + A^T w at the loop nodes in loop order, then one more column: -(g + A^T w)
                if (tid == 0) {
                    for (int m = 0; m < L; ++m) {
                        const double* mrec = REC + (size_t)kPgoRec * LP[3 * m];
                        double* gi = GR + 6 * (size_t)LP[3 * m + 1];
                        double* gj = GR + 6 * (size_t)LP[3 * m + 2];
                        for (int q = 0; q < 6; ++q) {
                            double si = 0.0, sj = 0.0;
                            for (int r = 0; r < 6; ++r) {
                                si += mrec[6 + 6 * r + q] * VA[6 * m + r];
                                sj += mrec[42 + 6 * r + q] * VA[6 * m + r];
                            }
                            gi[q] += si;
                            gj[q] += sj;
                        }
                    }
                    pgo_substitute(D, O, K, Z, zs, PgoColumn{0, 0, -1, -1, REC, GR});
                }
                __syncthreads();
            }
            for (int k = tid; k < K; k += kPgoThreads)
                for (int r = 0; r < 6; ++r) {
                    const double s = Z[(6 * (size_t)k + r) * zs];
                    mx = pgo_finite(s) ? fmax(mx, fabs(s)) : __builtin_inf();
                }
        }
        double* XO = X;                                // where the retraction writes
        if constexpr (!kLM) {
            dxmax = pgo_block_max(mx, red);
            if (!pgo_finite(dxmax)) { status = SSF_PGO_NOT_PD; break; }
        } else {
            dxt = pgo_block_max(mx, red);
            if (!pgo_finite(dxt)) {
                if (lm_invalid(it, kNaN)) break;
                continue;
            }
            // -- the model's decrease -(g^T dx + dx^T H dx / 2) = -sum_e (r_e . v_e + v_e . v_e / 2),
            //    v_e = Ji dx_i + Jj dx_j from the records of X: one thread per factor, a fixed-order sum
            double ms[1] = {0.0};
            for (int e = tid; e <= E; e += kPgoThreads) {
                const double* rec = REC + (size_t)kPgoRec * e;
                const int i = e < E ? IJ[2 * e] : 0, j = e < E ? IJ[2 * e + 1] : 0;
                double di[6], dj[6];
                for (int q = 0; q < 6; ++q) {
                    di[q] = e < E ? Z[(6 * (size_t)i + q) * zs] : 0.0;    // the prior has no Ji
                    dj[q] = Z[(6 * (size_t)j + q) * zs];
                }
                for (int r = 0; r < 6; ++r) {
                    double v = 0.0;
                    for (int q = 0; q < 6; ++q) v += rec[6 + 6 * r + q] * di[q] + rec[42 + 6 * r + q] * dj[q];
                    ms[0] -= rec[r] * v + 0.5 * v * v;
                }
            }
            block_sum<1>(ms, red);
            mcc = ms[0];
            if (!(mcc > 0.0)) {
                if (lm_invalid(it, mcc)) break;
                continue;
            }
            invalid = 0;
            trial = true;
            XO = XT;
        }
        for (int k = tid; k < K; k += kPgoThreads) {
            double d[6];
            for (int r = 0; r < 6; ++r) d[r] = Z[(6 * (size_t)k + r) * zs];
            const double* x = X + 7 * (size_t)k;
            double* xo = XO + 7 * (size_t)k;
            const double q[4] = {x[0], x[1], x[2], x[3]};
            double R[9];
            pgo_quat_R(q, R);
            for (int r = 0; r < 3; ++r) xo[4 + r] = x[4 + r] + (R[3 * r] * d[3] + R[3 * r + 1] * d[4] + R[3 * r + 2] * d[5]);
            const double th = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            const double sc = th < 1e-8 ? 0.5 : sin(0.5 * th) / th;
            const double dq[4] = {sc * d[0], sc * d[1], sc * d[2], th < 1e-8 ? 1.0 : cos(0.5 * th)};
            double qn[4];
            quat_mul(q, dq, qn);
            pgo_quat_unit(qn, qn);
            for (int c = 0; c < 4; ++c) xo[c] = qn[c];
        }
        __syncthreads();
        iters = it + 1;
    }

    if (status == SSF_PGO_OK || status == SSF_PGO_CONVERGED)
        for (int k = tid; k < K; k += kPgoThreads)
            for (int c = 0; c < 7; ++c) P[7 * (size_t)k + c] = X[7 * (size_t)k + c];
    if constexpr (kRobust)
        if (EO && status == SSF_PGO_NOT_PD)
            for (int e = tid; e < SSF_PGO_EDGE_OUT_STRIDE * E; e += kPgoThreads) EO[e] = kNaN;
    if constexpr (kLM) {
        if (EO && status != SSF_PGO_NOT_PD)            // (weight, s) at the last accepted point
            for (int e = tid; e < SSF_PGO_EDGE_OUT_STRIDE * E; e += kPgoThreads) EO[e] = WS[e];
        if (LL && status == SSF_PGO_NOT_PD)
            for (int k = tid; k < SSF_PGO_LM_LOG_STRIDE * max_iter; k += kPgoThreads) LL[k] = kNaN;
    }
    if (tid == 0) {
        const bool ok = status != SSF_PGO_NOT_PD;
        st[SSF_PGO_OUT_STATUS] = status; st[SSF_PGO_OUT_ITERATIONS] = ok ? iters : 0.0;
        st[SSF_PGO_OUT_COST0] = cost0; st[SSF_PGO_OUT_COST] = ok ? cost : kNaN;
        st[SSF_PGO_OUT_DX] = ok ? dxmax : 0.0; st[SSF_PGO_OUT_LOOPS] = L;
        st[SSF_PGO_OUT_ACCEPTED] = kLM && ok ? accepted : 0.0;
        st[SSF_PGO_OUT_RADIUS] = kLM && ok ? radius : 0.0;
    }
}

#define SSF_PGO_KERNEL_ARGS                                                                              \
    const PgoGraph *__restrict__ desc, double *__restrict__ pose, const int32_t *__restrict__ node_off,  \
        const int32_t *__restrict__ edge_ij, const double *__restrict__ edge_meas,                       \
        const double *__restrict__ edge_var, const int32_t *__restrict__ edge_off,                       \
        const double *__restrict__ prior_pose, const double *__restrict__ prior_var, int max_iter,       \
        double func_tol, double *scratch, double *__restrict__ stats, double *__restrict__ cost_log

__global__ __launch_bounds__(kPgoThreads) void k_pose_graph(SSF_PGO_KERNEL_ARGS) {
    pgo_solve<false, false>(desc, pose, node_off, edge_ij, edge_meas, edge_var, edge_off, prior_pose, prior_var,
                            max_iter, func_tol, scratch, stats, cost_log);
}

__global__ __launch_bounds__(kPgoThreads) void k_pose_graph_wide(SSF_PGO_KERNEL_ARGS) {
    pgo_solve<true, false>(desc, pose, node_off, edge_ij, edge_meas, edge_var, edge_off, prior_pose, prior_var,
                           max_iter, func_tol, scratch, stats, cost_log);
}

__global__ __launch_bounds__(kPgoThreads) void k_pose_graph_robust(SSF_PGO_KERNEL_ARGS, int rkind, double rk,
                                                                   double* __restrict__ edge_out) {
    pgo_solve<false, true>(desc, pose, node_off, edge_ij, edge_meas, edge_var, edge_off, prior_pose, prior_var,
                           max_iter, func_tol, scratch, stats, cost_log, rkind, rk, edge_out);
}

__global__ __launch_bounds__(kPgoThreads) void k_pose_graph_wide_robust(SSF_PGO_KERNEL_ARGS, int rkind, double rk,
                                                                        double* __restrict__ edge_out) {
    pgo_solve<true, true>(desc, pose, node_off, edge_ij, edge_meas, edge_var, edge_off, prior_pose, prior_var,
                          max_iter, func_tol, scratch, stats, cost_log, rkind, rk, edge_out);
}

// Step control: the loss kernels' arguments (kind none is weight 1), then the strategy and its log.
__global__ __launch_bounds__(kPgoThreads) void k_pose_graph_lm(SSF_PGO_KERNEL_ARGS, int rkind, double rk,
                                                               double* __restrict__ edge_out, ssf_pgo_lm lm,
                                                               double* __restrict__ lm_log) {
    pgo_solve<false, true, true>(desc, pose, node_off, edge_ij, edge_meas, edge_var, edge_off, prior_pose,
                                 prior_var, max_iter, func_tol, scratch, stats, cost_log, rkind, rk, edge_out, lm,
                                 lm_log);
}

__global__ __launch_bounds__(kPgoThreads) void k_pose_graph_wide_lm(SSF_PGO_KERNEL_ARGS, int rkind, double rk,
                                                                    double* __restrict__ edge_out, ssf_pgo_lm lm,
                                                                    double* __restrict__ lm_log) {
    pgo_solve<true, true, true>(desc, pose, node_off, edge_ij, edge_meas, edge_var, edge_off, prior_pose,
                                prior_var, max_iter, func_tol, scratch, stats, cost_log, rkind, rk, edge_out, lm,
                                lm_log);
}

// Both kernels run over every graph of the batch; a work-group returns at once when its graph
// (PgoGraph::wide) is the other kernel's.  A kernel with no graph of its own is not launched.
hipError_t launch_pose_graph(hipStream_t s, int n_graphs, bool any_narrow, bool any_wide, const PgoGraph* desc,
                             double* pose, const int32_t* node_off, const int32_t* edge_ij,
                             const double* edge_meas, const double* edge_var, const int32_t* edge_off,
                             const double* prior_pose, const double* prior_var, int max_iter,
                             double func_tol, double* scratch, double* stats, double* cost_log) {
    if (n_graphs <= 0) return hipSuccess;
    if (any_narrow) {
        kmark(s, "k_pose_graph");
        hipLaunchKernelGGL(k_pose_graph, dim3(n_graphs), dim3(kPgoThreads), 0, s, desc, pose, node_off, edge_ij,
                           edge_meas, edge_var, edge_off, prior_pose, prior_var, max_iter, func_tol, scratch,
                           stats, cost_log);
    }
    if (any_wide) {
        kmark(s, "k_pose_graph_wide");
        hipLaunchKernelGGL(k_pose_graph_wide, dim3(n_graphs), dim3(kPgoThreads), 0, s, desc, pose, node_off,
                           edge_ij, edge_meas, edge_var, edge_off, prior_pose, prior_var, max_iter, func_tol,
                           scratch, stats, cost_log);
    }
    return hipGetLastError();
}

// The same dispatch onto the kernels with a loss on the loop edges and the per-edge output.
hipError_t launch_pose_graph_robust(hipStream_t s, int n_graphs, bool any_narrow, bool any_wide,
                                    const PgoGraph* desc, double* pose, const int32_t* node_off,
                                    const int32_t* edge_ij, const double* edge_meas, const double* edge_var,
                                    const int32_t* edge_off, const double* prior_pose, const double* prior_var,
                                    int max_iter, double func_tol, double* scratch, double* stats,
                                    double* cost_log, int rkind, double rk, double* edge_out) {
    if (n_graphs <= 0) return hipSuccess;
    if (any_narrow) {
        kmark(s, "k_pose_graph_robust");
        hipLaunchKernelGGL(k_pose_graph_robust, dim3(n_graphs), dim3(kPgoThreads), 0, s, desc, pose, node_off,
                           edge_ij, edge_meas, edge_var, edge_off, prior_pose, prior_var, max_iter, func_tol,
                           scratch, stats, cost_log, rkind, rk, edge_out);
    }
    if (any_wide) {
        kmark(s, "k_pose_graph_wide_robust");
        hipLaunchKernelGGL(k_pose_graph_wide_robust, dim3(n_graphs), dim3(kPgoThreads), 0, s, desc, pose,
                           node_off, edge_ij, edge_meas, edge_var, edge_off, prior_pose, prior_var, max_iter,
                           func_tol, scratch, stats, cost_log, rkind, rk, edge_out);
    }
    return hipGetLastError();
}

// The same dispatch onto the kernels with step control; the scratch is sized with lm = true.
hipError_t launch_pose_graph_lm(hipStream_t s, int n_graphs, bool any_narrow, bool any_wide, const PgoGraph* desc,
                                double* pose, const int32_t* node_off, const int32_t* edge_ij,
                                const double* edge_meas, const double* edge_var, const int32_t* edge_off,
                                const double* prior_pose, const double* prior_var, int max_iter, double func_tol,
                                double* scratch, double* stats, double* cost_log, int rkind, double rk,
                                double* edge_out, const ssf_pgo_lm& lm, double* lm_log) {
    if (n_graphs <= 0) return hipSuccess;
    if (any_narrow) {
        kmark(s, "k_pose_graph_lm");
        hipLaunchKernelGGL(k_pose_graph_lm, dim3(n_graphs), dim3(kPgoThreads), 0, s, desc, pose, node_off, edge_ij,
                           edge_meas, edge_var, edge_off, prior_pose, prior_var, max_iter, func_tol, scratch,
                           stats, cost_log, rkind, rk, edge_out, lm, lm_log);
    }
    if (any_wide) {
        kmark(s, "k_pose_graph_wide_lm");
        hipLaunchKernelGGL(k_pose_graph_wide_lm, dim3(n_graphs), dim3(kPgoThreads), 0, s, desc, pose, node_off,
                           edge_ij, edge_meas, edge_var, edge_off, prior_pose, prior_var, max_iter, func_tol,
                           scratch, stats, cost_log, rkind, rk, edge_out, lm, lm_log);
    }
    return hipGetLastError();
}

}  // namespace ssf
