// pgo_step.hpp -- the ends of the pose-graph solver and what its iteration loop carries: the
// prologue (validation, the loop list, the graph's scratch), the Gauss-Newton and the
// Levenberg-Marquardt bookkeeping of an evaluated point, the model decrease, the retraction, and
// the epilogue (poses, per-edge output and statistics).
#pragma once
#include "pgo_common.hpp"

namespace ssf {

// what the iteration loop carries from pass to pass, uniform over the work-group
struct PgoIter {
    int iters = 0, status = SSF_PGO_OK;
    double cost0 = 0.0, cost = 0.0, prev = 0.0, dxmax = 0.0;
};

// Validation before any indexed access, the loop edges in edge order (wide: into the graph's
// scratch, narrow: into LDS), the context c, and the working copy X of the poses (unit
// quaternions).  -> false when the work-group is done: its graph belongs to the other kernel, or
// it failed validation (status and NaN outputs written here).  Every loop bound of the stages is
// a count validated here (K, E from the host descriptor checked against the device offsets,
// L <= lcap <= SSF_PGO_MAX_LOOPS).
template <bool kWide, bool kRobust, bool kLM>
SSF_DEV bool pgo_prologue(const PgoArgs& a, PgoLds<kWide>& S, PgoCtx& c) {
    const int g = blockIdx.x, tid = threadIdx.x;
    const PgoGraph G = a.desc[g];
    if ((G.wide != 0) != kWide) return false;
    const int K = G.K, E = G.E, max_iter = a.max_iter;
    double* base = a.scratch + G.scratch_off;
    const PgoLayout lay(K, E, G.lcap, kWide, kLM);
    int32_t* LP = reinterpret_cast<int32_t*>(base + lay.LP);
    const int lmax = kWide ? G.lcap : kPgoNarrowLoops;
    double* st = a.stats + (size_t)g * SSF_PGO_OUT_STRIDE;
    double* clog = a.cost_log ? a.cost_log + (size_t)g * (size_t)(max_iter + 1) : nullptr;
    const double kNaN = __builtin_nan("");
    // the host validated its edge offsets against each other: the call's output has E rows from edge0
    double* EO = kRobust && a.edge_out ? a.edge_out + (size_t)SSF_PGO_EDGE_OUT_STRIDE * (size_t)G.edge0 : nullptr;
    double* LL = kLM && a.lm_log ? a.lm_log + (size_t)g * (size_t)max_iter * SSF_PGO_LM_LOG_STRIDE : nullptr;

    if (tid == 0) { S.bad = 0; S.nloop = 0; S.fail = 0; }
    __syncthreads();
    if (clog)
        for (int k = tid; k <= max_iter; k += kPgoThreads) clog[k] = kNaN;
    if constexpr (kLM)
        if (LL)
            for (int k = tid; k < SSF_PGO_LM_LOG_STRIDE * max_iter; k += kPgoThreads) LL[k] = kNaN;
    int status = -1;
    if (K == 0) status = SSF_PGO_EMPTY;
    if (a.node_off[g] != G.node0 || a.node_off[g + 1] != G.node0 + K || a.edge_off[g] != G.edge0 ||
        a.edge_off[g + 1] != G.edge0 + E)
        status = SSF_PGO_BAD_INPUT;              // the device offsets disagree with the host's
    double* P = a.pose + 7 * (size_t)G.node0;
    const int32_t* IJ = a.edge_ij + 2 * (size_t)G.edge0;
    const double* ZM = a.edge_meas + 7 * (size_t)G.edge0;
    const double* ZV = a.edge_var + 6 * (size_t)G.edge0;
    const double* PP = a.prior_pose + 7 * (size_t)g;
    const double* PV = a.prior_var + 6 * (size_t)g;
    if (status < 0) {
        int bad = 0;
        for (int k = tid; k < K; k += kPgoThreads) {
            const double* p = P + 7 * (size_t)k;
            for (int q = 0; q < 7; ++q) bad |= !pgo_finite(p[q]);
            bad |= !(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3] > 0.0);
        }
        for (int e = tid; e < E; e += kPgoThreads) {
            const int i = IJ[2 * e], j = IJ[2 * e + 1];
            bad |= (i < 0 || i >= K || j < 0 || j >= K || i == j);
            const double* z = ZM + 7 * (size_t)e;
            for (int q = 0; q < 7; ++q) bad |= !pgo_finite(z[q]);
            bad |= !(z[0] * z[0] + z[1] * z[1] + z[2] * z[2] + z[3] * z[3] > 0.0);
            for (int q = 0; q < 6; ++q) bad |= !(pgo_finite(ZV[6 * (size_t)e + q]) && ZV[6 * (size_t)e + q] > 0.0);
        }
        if (tid < 7) bad |= !pgo_finite(PP[tid]);
        if (tid == 7) bad |= !(PP[0] * PP[0] + PP[1] * PP[1] + PP[2] * PP[2] + PP[3] * PP[3] > 0.0);
        if (tid >= 8 && tid < 14) bad |= !(pgo_finite(PV[tid - 8]) && PV[tid - 8] > 0.0);
        if (bad) atomicOr(&S.bad, 1);
        __syncthreads();
        if (S.bad) status = SSF_PGO_BAD_INPUT;
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
                    else { S.loop_e[pos] = e; S.loop_i[pos] = i; S.loop_j[pos] = j; }
                }
                cnt += __popcll(m);
            }
            if (tid == 0) S.nloop = cnt;
        }
        __syncthreads();
        L = S.nloop;
        if (L > SSF_PGO_MAX_LOOPS) status = SSF_PGO_TOO_MANY_LOOPS;
        // fewer than K - 1 chain edges: some (k, k + 1) pair is unlinked and T is singular
        else if (L > G.lcap) status = SSF_PGO_NOT_PD;
    }
    if (status >= 0) {
        if (tid == 0) {
            st[SSF_PGO_OUT_STATUS] = status; st[SSF_PGO_OUT_ITERATIONS] = 0.0;
            st[SSF_PGO_OUT_COST0] = kNaN; st[SSF_PGO_OUT_COST] = kNaN;
            st[SSF_PGO_OUT_DX] = 0.0; st[SSF_PGO_OUT_LOOPS] = status == SSF_PGO_EMPTY || status == SSF_PGO_BAD_INPUT ? 0.0 : (double)S.nloop;
            st[6] = 0.0; st[7] = 0.0;
        }
        if constexpr (kRobust)
            if (EO)
                for (int e = tid; e < SSF_PGO_EDGE_OUT_STRIDE * E; e += kPgoThreads) EO[e] = kNaN;
        return false;
    }

    c.tid = tid; c.K = K; c.E = E; c.L = L; c.n = 6 * L; c.NC = 6 * L + 1; c.max_iter = max_iter;
    c.rkind = a.rkind; c.rk = a.rk; c.func_tol = a.func_tol;
    c.zs = kWide ? (size_t)kPgoThreads : (size_t)c.NC;
    c.P = P; c.IJ = IJ; c.ZM = ZM; c.ZV = ZV; c.PP = PP; c.PV = PV; c.LP = LP;
    c.X = base + lay.X; c.REC = base + lay.REC; c.D = base + lay.D; c.O = base + lay.O; c.GR = base + lay.GR;
    c.Z = base + lay.Z; c.CM = base + lay.CM; c.VA = base + lay.VA; c.VB = base + lay.VB;
    c.XT = base + lay.XT; c.RECT = base + lay.RECT; c.WS = base + lay.WS; c.WST = base + lay.WST;
    c.st = st; c.clog = clog; c.EO = EO; c.LL = LL;
    for (int k = tid; k < K; k += kPgoThreads) {
        double q[4];
        pgo_quat_unit(P + 7 * (size_t)k, q);
        for (int r = 0; r < 4; ++r) c.X[7 * (size_t)k + r] = q[r];
        for (int r = 4; r < 7; ++r) c.X[7 * (size_t)k + r] = P[7 * (size_t)k + r];
    }
    __syncthreads();
    return true;
}

// Gauss-Newton: the cost of pass `it` -> true when the graph stops here (the evaluation after
// the last retraction, or converged).
SSF_DEV bool pgo_gn_evaluate(const PgoCtx& c, PgoIter& I, int it, double cost) {
    I.cost = cost;
    if (c.tid == 0 && c.clog) c.clog[it] = cost;
    if (it == 0) I.cost0 = cost;
    if (it == c.max_iter) return true;
    if (it > 0 && c.func_tol > 0.0 && fabs(I.prev - cost) <= c.func_tol * I.prev) { I.status = SSF_PGO_CONVERGED; return true; }
    I.prev = cost;
    return false;
}

// Levenberg-Marquardt step control (ssf_pgo_lm; Ceres' LevenbergMarquardtStrategy, as k_solve's),
// uniform over the work-group.  One pass of the loop is one attempt: T gets D / radius on its
// diagonal, the step goes to the trial poses XT, and the next pass linearises the trial point and
// accepts it (the pose, record and weight buffers swap with their trial twins) or rejects it.
// Without step control there is no state at all, so those kernels carry none of it.
template <bool kLM>
struct PgoLm {
    static constexpr double radius = 0.0;          // pgo_assemble<false> does not read it
    SSF_DEV explicit PgoLm(const ssf_pgo_lm&) {}
};
template <>
struct PgoLm<true> {
    ssf_pgo_lm prm;
    double radius, dec = 2.0;      // the trust-region radius, what the next rejection divides it by
    double mcc = 0.0, dxt = 0.0;   // the model decrease and the max-norm of the step that waits in XT
    int invalid_run = 0, accepted = 0;
    bool trial = false;            // XT holds a trial point that waits for its evaluation
    SSF_DEV explicit PgoLm(const ssf_pgo_lm& p) : prm(p), radius(p.radius0) {}

    SSF_DEV void reject() {
        radius /= dec;
        dec *= 2.0;
    }
    // the trial point becomes the point -> true when the cost fell by no more than func_tol of it
    SSF_DEV bool accept(PgoCtx& c, PgoIter& I, double ct, double rho) {
        I.prev = I.cost;
        I.cost = ct;
        double* sw = c.X; c.X = c.XT; c.XT = sw;
        sw = c.REC; c.REC = c.RECT; c.RECT = sw;
        sw = c.WS; c.WS = c.WST; c.WST = sw;
        ++accepted;
        I.dxmax = dxt;
        const double t = 2.0 * rho - 1.0;
        radius = fmin(radius / fmax(1.0 / 3.0, 1.0 - t * t * t), prm.max_radius);
        dec = 2.0;
        return c.func_tol > 0.0 && I.prev - I.cost <= c.func_tol * I.prev;
    }
    // an attempt without a usable step (a pivot of the damped system failed, a non-finite step,
    // no model decrease m): the radius shrinks, the point stays -> true after more than 5 in a row
    SSF_DEV bool invalid(const PgoCtx& c, PgoIter& I, int it, double m) {
        reject();
        trial = false;
        I.iters = it + 1;
        if (c.tid == 0) {
            if (c.clog) c.clog[it + 1] = I.cost;
            if (c.LL) {
                double* ll = c.LL + (size_t)SSF_PGO_LM_LOG_STRIDE * it;
                ll[SSF_PGO_LM_LOG_MCC] = m; ll[SSF_PGO_LM_LOG_RADIUS] = radius;
                ll[SSF_PGO_LM_LOG_OUTCOME] = SSF_PGO_LM_INVALID;
            }
        }
        return ++invalid_run > 5;
    }
    // The cost ct of what pass `it` linearised: the start (pass 0), or the trial point of attempt
    // `it`, which is accepted when the cost fell by more than min_relative_decrease of what the
    // model promised (a NaN trial cost rejects) -> true when the graph stops here.
    SSF_DEV bool evaluate(PgoCtx& c, PgoIter& I, int it, double ct) {
        if (it == 0) {
            I.cost = I.cost0 = ct;
            if (c.tid == 0 && c.clog) c.clog[0] = ct;
        } else if (trial) {
            const double rho = (I.cost - ct) / mcc;
            const bool acc = rho > prm.min_relative_decrease;
            bool stop = false;
            if (acc) {
                if (accept(c, I, ct, rho)) { I.status = SSF_PGO_CONVERGED; stop = true; }
            } else {
                reject();
            }
            trial = false;
            if (c.tid == 0) {
                if (c.clog) c.clog[it] = I.cost;
                if (c.LL) {
                    double* ll = c.LL + (size_t)SSF_PGO_LM_LOG_STRIDE * (it - 1);
                    ll[SSF_PGO_LM_LOG_COST] = ct; ll[SSF_PGO_LM_LOG_MCC] = mcc;
                    ll[SSF_PGO_LM_LOG_RADIUS] = radius;
                    ll[SSF_PGO_LM_LOG_OUTCOME] = acc ? SSF_PGO_LM_ACCEPTED : SSF_PGO_LM_REJECTED;
                }
            }
            if (stop || radius < prm.min_radius) return true;
        }
        return it == c.max_iter;
    }
};

// The model's decrease -(g^T dx + dx^T H dx / 2) = -sum_e (r_e . v_e + v_e . v_e / 2) of the step
// in column 0 of Z, v_e = Ji dx_i + Jj dx_j from the records of X: one thread per factor, a
// fixed-order sum, on every thread.
SSF_DEV double pgo_model_decrease(const PgoCtx& c, PgoLdsCommon& S) {
    const int E = c.E;
    const size_t zs = c.zs;
    double ms[1] = {0.0};
    for (int e = c.tid; e <= E; e += kPgoThreads) {
        const double* rec = c.REC + (size_t)kPgoRec * e;
        const int i = e < E ? c.IJ[2 * e] : 0, j = e < E ? c.IJ[2 * e + 1] : 0;
        double di[6], dj[6];
        for (int q = 0; q < 6; ++q) {
            di[q] = e < E ? c.Z[(6 * (size_t)i + q) * zs] : 0.0;    // the prior has no Ji
            dj[q] = c.Z[(6 * (size_t)j + q) * zs];
        }
        for (int r = 0; r < 6; ++r) {
            double v = 0.0;
            for (int q = 0; q < 6; ++q) v += rec[6 + 6 * r + q] * di[q] + rec[42 + 6 * r + q] * dj[q];
            ms[0] -= rec[r] * v + 0.5 * v * v;
        }
    }
    block_sum<1>(ms, S.red);
    return ms[0];
}

// XO = X (+) dx, dx in column 0 of Z: one thread per node.  Ends with a barrier.
SSF_DEV void pgo_retract(const PgoCtx& c, double* XO) {
    for (int k = c.tid; k < c.K; k += kPgoThreads) {
        double d[6];
        for (int r = 0; r < 6; ++r) d[r] = c.Z[(6 * (size_t)k + r) * c.zs];
        const double* x = c.X + 7 * (size_t)k;
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
        for (int r = 0; r < 4; ++r) xo[r] = qn[r];
    }
    __syncthreads();
}

// The poses go back only from a graph that ends SSF_PGO_OK / SSF_PGO_CONVERGED; a graph that
// fails (SSF_PGO_NOT_PD) gets NaN per-edge output and step log.
template <bool kRobust, bool kLM>
SSF_DEV void pgo_epilogue(const PgoCtx& c, const PgoIter& I, const PgoLm<kLM>& lm) {
    const int tid = c.tid, K = c.K, E = c.E, status = I.status;
    const double kNaN = __builtin_nan("");
    if (status == SSF_PGO_OK || status == SSF_PGO_CONVERGED)
        for (int k = tid; k < K; k += kPgoThreads)
            for (int q = 0; q < 7; ++q) c.P[7 * (size_t)k + q] = c.X[7 * (size_t)k + q];
    if constexpr (kRobust)
        if (c.EO && status == SSF_PGO_NOT_PD)
            for (int e = tid; e < SSF_PGO_EDGE_OUT_STRIDE * E; e += kPgoThreads) c.EO[e] = kNaN;
    if constexpr (kLM) {
        if (c.EO && status != SSF_PGO_NOT_PD)          // (weight, s) at the last accepted point
            for (int e = tid; e < SSF_PGO_EDGE_OUT_STRIDE * E; e += kPgoThreads) c.EO[e] = c.WS[e];
        if (c.LL && status == SSF_PGO_NOT_PD)
            for (int k = tid; k < SSF_PGO_LM_LOG_STRIDE * c.max_iter; k += kPgoThreads) c.LL[k] = kNaN;
    }
    if (tid == 0) {
        const bool ok = status != SSF_PGO_NOT_PD;
        double* st = c.st;
        st[SSF_PGO_OUT_STATUS] = status; st[SSF_PGO_OUT_ITERATIONS] = ok ? I.iters : 0.0;
        st[SSF_PGO_OUT_COST0] = I.cost0; st[SSF_PGO_OUT_COST] = ok ? I.cost : kNaN;
        st[SSF_PGO_OUT_DX] = ok ? I.dxmax : 0.0; st[SSF_PGO_OUT_LOOPS] = c.L;
        if constexpr (kLM) {
            st[SSF_PGO_OUT_ACCEPTED] = ok ? lm.accepted : 0.0;
            st[SSF_PGO_OUT_RADIUS] = ok ? lm.radius : 0.0;
        } else {
            st[SSF_PGO_OUT_ACCEPTED] = 0.0;
            st[SSF_PGO_OUT_RADIUS] = 0.0;
        }
    }
}

}  // namespace ssf
