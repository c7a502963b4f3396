// pgo_linearise.hpp -- the linearise phase of the pose-graph solver: one thread per factor writes
// the whitened residual and the two Jacobians (a record of kPgoRec doubles), applies the loss to
// a loop edge, and the work-group sums the cost.
#pragma once
#include "pgo_common.hpp"

namespace ssf {

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

// Linearise every factor at the poses Xl into the records Rl (factor E is the prior) -> the sum
// of s (kRobust: of 2 rho(s)) over the factors, on every thread; its barriers also publish Rl.
// lin = false: nothing to linearise (step control after an attempt without a step), the sum is 0.
// kRobust: a loop edge's record is scaled by sqrt(w(s)) in place (what the assemble phase,
// PgoColumn and the capacitance read), and (w, s) of every edge go to Wl under step control (edge_out
// gets the accepted point's at the end), to edge_out without it.
template <bool kRobust, bool kLM>
SSF_DEV double pgo_linearise_all(const PgoCtx& c, PgoLdsCommon& S, const double* Xl, double* Rl, double* Wl, bool lin) {
    const int E = c.E;
    double cs[1] = {0.0};
    for (int e = lin ? c.tid : E + 1; e <= E; e += kPgoThreads) {
        double* rec = Rl + (size_t)kPgoRec * e;
        if (e < E) {
            const double* xi = Xl + 7 * (size_t)c.IJ[2 * e];
            const double* xj = Xl + 7 * (size_t)c.IJ[2 * e + 1];
            pgo_linearise(xi, xi + 4, xj, xj + 4, c.ZM + 7 * (size_t)e, c.ZV + 6 * (size_t)e, rec);
        } else {
            const double qi[4] = {0.0, 0.0, 0.0, 1.0}, ti[3] = {0.0, 0.0, 0.0};
            pgo_linearise(qi, ti, Xl, Xl + 4, c.PP, c.PV, rec);
        }
        double s = 0.0;
        for (int q = 0; q < 6; ++q) s += rec[q] * rec[q];
        if constexpr (kRobust) {
            double w = 1.0, rho2 = s;
            if (e < E) {
                const int i = c.IJ[2 * e], j = c.IJ[2 * e + 1];
                if (i - j != 1 && j - i != 1) {
                    const double2 wr = pgo_robust_loss(c.rkind, c.rk, s);
                    w = wr.x;
                    rho2 = wr.y;
                    const double sw = sqrt(w);
                    for (int q = 0; q < kPgoRec; ++q) rec[q] *= sw;
                }
                if constexpr (kLM) {
                    Wl[SSF_PGO_EDGE_OUT_STRIDE * (size_t)e + SSF_PGO_EDGE_WEIGHT] = w;
                    Wl[SSF_PGO_EDGE_OUT_STRIDE * (size_t)e + SSF_PGO_EDGE_CHI2] = s;
                } else if (c.EO) {
                    c.EO[SSF_PGO_EDGE_OUT_STRIDE * (size_t)e + SSF_PGO_EDGE_WEIGHT] = w;
                    c.EO[SSF_PGO_EDGE_OUT_STRIDE * (size_t)e + SSF_PGO_EDGE_CHI2] = s;
                }
            }
            cs[0] += rho2;
        } else {
            cs[0] += s;
        }
    }
    block_sum<1>(cs, S.red);
    return cs[0];
}

}  // namespace ssf
