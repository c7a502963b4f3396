// pose_graph.hip -- the pose-graph optimisation of mapOptmization (runOptimize,
// src/mapOptmization.cpp:280-293, over the factors of :147-165,274) on gfx950: batched
// Gauss-Newton on SE(3), one work-group per graph, the whole iteration loop on the device.
//
//   poses        7 doubles, q(x, y, z, w) then t; tangent = (rotation, translation), GTSAM's
//                Pose3 order; retraction X (+) d = X * [Exp(w), v] (right-multiplied, first-order
//                translation: GTSAM's chart with GTSAM_POSE3_EXPMAP off).
//   factors      between (i, j, Z, var): E = Z^-1 Xi^-1 Xj, r = [Log(R_E); t_E] / sigma;
//                prior (P, var) on node 0: the same with Xi = identity, Z = P.
//   per iteration (every stage is work-group wide, separated by barriers; pgo_solve lists them):
//     linearise  one thread per factor: whitened residual and the two 6x6 Jacobians (pgo_linearise.hpp)
//     assemble   one thread per node walks the edge list in order (fixed summation order, no
//                floating-point atomics): the gradient over every factor, and the block-tridiagonal
//                part T (prior + edges with |i - j| == 1)
//     factor     block Cholesky of T, serial over the nodes on one lane (depth K)
//     substitute one lane per right-hand side: -g and the 6 L columns of A^T, A = the whitened
//                Jacobian rows of the L loop edges (every edge with |i - j| != 1); forward and
//                back substitution, serial over the nodes (the three: pgo_tridiag.hpp)
//     Woodbury   capacitance C = I + A T^-1 A^T (6L x 6L), dense Cholesky,
//                dx = T^-1 b - T^-1 A^T C^-1 A T^-1 b (pgo_capacitance.hpp)
//     retract    one thread per node (pgo_step.hpp, with the prologue, the bookkeeping and the epilogue)
//   The above is k_pose_graph, for graphs with at most 32 edges beyond the K - 1 of a chain
//   (so at most 32 loop edges): one lane per column, one thread per row of C, the loop list and
//   the capacitance vectors in LDS.  Every other graph is k_pose_graph_wide's (up to
//   SSF_PGO_MAX_LOOPS loop edges): the columns go through kPgoThreads at a time and are folded
//   into C pass by pass, and the loop list, C and its vectors live in the graph's scratch
//   (PgoLayout, pgo_common.hpp).  The host picks the kernel (PgoGraph::wide, from K and E).
//   k_pose_graph_robust / k_pose_graph_wide_robust are the same two solvers with an m-estimator on
//   the loop edges (ssf_pgo_robust; IRLS, Triggs' first-order form): at every linearisation a loop
//   edge's record is scaled by sqrt(w(s)), s its squared whitened residual, and it enters the cost
//   with 2 rho(s).  Chain edges and the prior stay quadratic, so T is what it is without the loss.
//   They also report every edge's weight and s (edge_out).
//   k_pose_graph_lm / k_pose_graph_wide_lm are the loss kernels with Levenberg-Marquardt step control
//   (ssf_pgo_lm): T is damped by D / radius, the step goes to a trial point, and only a trial that
//   lowers the cost by enough of what the model promised becomes the point (PgoLm, pgo_step.hpp).
//   No inter-work-group communication of any kind.  A graph writes its poses back only when it
//   ends with SSF_PGO_OK / SSF_PGO_CONVERGED: it iterates on a copy in the context scratch.
#include "pgo_common.hpp"
#include "pgo_linearise.hpp"
#include "pgo_tridiag.hpp"
#include "pgo_capacitance.hpp"
#include "pgo_step.hpp"

namespace ssf {

bool pgo_graph_wide(int K, int E) { return E - (K - 1) > kPgoNarrowLoops; }

size_t pgo_graph_doubles(int K, int E, int lcap, bool wide, bool lm) { return PgoLayout(K, E, lcap, wide, lm).total; }

// The solver of all six kernels.  kWide: which of the two paths; a work-group whose graph belongs
// to the other kernel returns at once.  kRobust: the loss (rkind, rk) on the loop edges, and
// edge_out: two doubles per edge (SSF_PGO_EDGE_*) at the host's edge offsets, NaN for a graph
// that fails.  kLM: step control; one pass of the loop is then one attempt, and lm_log gets
// SSF_PGO_LM_LOG_STRIDE doubles per attempt, NaN for a graph that fails.
template <bool kWide, bool kRobust, bool kLM = false>
SSF_DEV void pgo_solve(const PgoArgs& a) {
    __shared__ PgoLds<kWide> S;
    PgoCtx c;
    if (!pgo_prologue<kWide, kRobust, kLM>(a, S, c)) return;
    const double kNaN = __builtin_nan("");
    PgoIter I;
    PgoLm<kLM> lm(a.lm);
    for (int it = 0; it <= c.max_iter; ++it) {
        // -- linearise and evaluate.  Step control: pass 0 linearises the start, a later pass the
        //    trial point of the attempt before it (none after an invalid attempt)
        if constexpr (!kLM) {
            const double cs = pgo_linearise_all<kRobust, false>(c, S, c.X, c.REC, nullptr, true);
            if (pgo_gn_evaluate(c, I, it, 0.5 * cs)) break;
        } else {
            const bool at0 = it == 0;
            const double cs = pgo_linearise_all<kRobust, true>(c, S, at0 ? c.X : c.XT, at0 ? c.REC : c.RECT,
                                                               at0 ? c.WS : c.WST, at0 || lm.trial);
            if (lm.evaluate(c, I, it, 0.5 * cs)) break;
        }

        // -- T and the gradient, then T's factors
        pgo_assemble<kLM>(c, S, lm.radius);
        pgo_block_cholesky<kLM>(c, S);
        if constexpr (kLM) {
            // a missing chain link ends the graph as without step control (damping would make
            // that singular T factorable); a failed pivot of the damped T is an invalid step
            const int f = S.fail;
            if (f & 1) { I.status = SSF_PGO_NOT_PD; break; }
            if (f) {
                __syncthreads();
                if (c.tid == 0) S.fail = 0;
                __syncthreads();
                if (lm.invalid(c, I, it, kNaN)) break;
                continue;
            }
        } else {
            if (S.fail) { I.status = SSF_PGO_NOT_PD; break; }
        }

        // -- the step dx, into column 0 of Z; a failed pivot of C is no step
        double mx = 0.0;
        bool failed;
        if constexpr (kWide) failed = pgo_capacitance_wide(c, S, mx);
        else failed = pgo_capacitance_narrow(c, S, mx);
        if (failed) {
            if constexpr (kLM) {
                if (lm.invalid(c, I, it, kNaN)) break;
                continue;
            }
            I.status = SSF_PGO_NOT_PD;
            break;
        }

        // -- retract: onto the point, or under step control onto the trial point
        double* XO = c.X;
        if constexpr (!kLM) {
            I.dxmax = pgo_block_max(mx, S.red);
            if (!pgo_finite(I.dxmax)) { I.status = SSF_PGO_NOT_PD; break; }
        } else {
            lm.dxt = pgo_block_max(mx, S.red);
            if (!pgo_finite(lm.dxt)) {
                if (lm.invalid(c, I, it, kNaN)) break;
                continue;
            }
            lm.mcc = pgo_model_decrease(c, S);
            if (!(lm.mcc > 0.0)) {
                if (lm.invalid(c, I, it, lm.mcc)) break;
                continue;
            }
            lm.invalid_run = 0;
            lm.trial = true;
            XO = c.XT;
        }
        pgo_retract(c, XO);
        I.iters = it + 1;
    }
    pgo_epilogue<kRobust, kLM>(c, I, lm);
}

__global__ __launch_bounds__(kPgoThreads) void k_pose_graph(PgoArgs a) { pgo_solve<false, false>(a); }
__global__ __launch_bounds__(kPgoThreads) void k_pose_graph_wide(PgoArgs a) { pgo_solve<true, false>(a); }
__global__ __launch_bounds__(kPgoThreads) void k_pose_graph_robust(PgoArgs a) { pgo_solve<false, true>(a); }
__global__ __launch_bounds__(kPgoThreads) void k_pose_graph_wide_robust(PgoArgs a) { pgo_solve<true, true>(a); }
__global__ __launch_bounds__(kPgoThreads) void k_pose_graph_lm(PgoArgs a) { pgo_solve<false, true, true>(a); }
__global__ __launch_bounds__(kPgoThreads) void k_pose_graph_wide_lm(PgoArgs a) { pgo_solve<true, true, true>(a); }

// Both kernels of the pair (a.has_lm: step control, else a.robust: the loss, else plain) run over
// every graph of the batch; a work-group returns at once when its graph (PgoGraph::wide) is the
// other kernel's.  A kernel with no graph of its own is not launched.
hipError_t launch_pose_graph(hipStream_t s, int n_graphs, bool any_narrow, bool any_wide, const PgoArgs& a) {
    if (n_graphs <= 0) return hipSuccess;
    using Kernel = void (*)(PgoArgs);
    struct Pair { Kernel narrow, wide; const char *narrow_name, *wide_name; };
    const Pair p = a.has_lm   ? Pair{k_pose_graph_lm, k_pose_graph_wide_lm, "k_pose_graph_lm", "k_pose_graph_wide_lm"}
                   : a.robust ? Pair{k_pose_graph_robust, k_pose_graph_wide_robust, "k_pose_graph_robust", "k_pose_graph_wide_robust"}
                              : Pair{k_pose_graph, k_pose_graph_wide, "k_pose_graph", "k_pose_graph_wide"};
    if (any_narrow) {
        kmark(s, p.narrow_name);
        hipLaunchKernelGGL(p.narrow, dim3(n_graphs), dim3(kPgoThreads), 0, s, a);
    }
    if (any_wide) {
        kmark(s, p.wide_name);
        hipLaunchKernelGGL(p.wide, dim3(n_graphs), dim3(kPgoThreads), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace ssf
