// mask_gmm.hpp -- the small dense algebra of the GMM fit of k_mask_pose: the M-step and the
// E-step's difference form on two lanes (gmm_params2), and the per-point E-step pieces.
#pragma once
#include "mask_common.hpp"

namespace ssf {

// The E-step in difference form (gmm_params2).  With P_k = U_k U_k^T, v = x - s (s = S.mean) and
// m_k = mu_k - s, sklearn's weighted log-probabilities a_k = -0.5 (v - m_k)' P_k (v - m_k) + K_k,
// K_k = -3 log(2 pi) + logdet_k + logw_k, differ by the quadratic
//     delta = a1 - a0 = v' A v + b' v + c,   A = -0.5 (P1 - P0),  b = P1 m1 - P0 m0,
//     c = -0.5 (m1' P1 m1 - m0' P0 m0) + K1 - K0,
// which is all the per-point work needs: resp1 = sigmoid(delta), argmax = [delta > 0], and
// logsumexp(a0, a1) = a0 + max(delta, 0) + log1p(exp(-|delta|)).  The a0 part of the lower bound
// is summed over the frame from the pass-0 moments about s (S.tot = {N, M1, M2}):
//     sum_i a0_i = N K0 - 0.5 (tr(P0 M2) - 2 m0' P0 M1 + N m0' P0 m0).
// Aq is packed upper with the off-diagonal entries doubled (v'Av = sum_j v_j sum_{k>=j} Aq_jk v_k).

// ---- the M-step algebra on two lanes -------------------------------------------------------
// sklearn _estimate_gaussian_parameters + _compute_precision_cholesky + the difference form
// above, between passes: component k on lane k of wave 0 (both lanes run one instruction
// stream, so two components cost one) with every 6x6 quantity in registers (fully unrolled).
// Round 2 ran the same operations in the same order on lane 0 over LDS arrays, element by
// element (40-53 k cycles per EM pass); the outputs are bit-identical to that version on a
// 256-frame batch (every output double, every mask byte), and the launch is 4 % shorter.

// C (6x6, row-major) -> precision Cholesky, packed upper U, and its log det: scipy
// linalg.cholesky(lower) + solve_triangular(L, I).T as sklearn _compute_precision_cholesky.
SSF_DEV int prec_chol6_r(const double (&C)[36], double (&U)[21], double& logdet) {
    double L[36], Li[36];
#pragma unroll
    for (int k = 0; k < 36; ++k) { L[k] = 0.0; Li[k] = 0.0; }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = C[j * 6 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[j * 6 + k] * L[j * 6 + k];
        ok = ok && (s > 0.0);
        L[j * 6 + j] = sqrt(s);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = C[i * 6 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i * 6 + k] * L[j * 6 + k];
            L[i * 6 + j] = v / L[j * 6 + j];
        }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int i = c; i < 6; ++i) {
            double v = (i == c) ? 1.0 : 0.0;
#pragma unroll
            for (int k = c; k < i; ++k) v -= L[i * 6 + k] * Li[k * 6 + c];
            Li[i * 6 + c] = v / L[i * 6 + i];
        }
    double ld = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) U[up(i, j)] = Li[j * 6 + i];
#pragma unroll
    for (int i = 0; i < 6; ++i) ld += log(Li[i * 6 + i]);
    logdet = ld;
    return ok ? 0 : -1;
}

// Lanes 0 and 1 of wave 0 (lane k: component k): the M-step and the difference form.  Returns, in lane 0,
// -1 when a covariance is not positive definite (the parameters are then left as they were).
__device__ __noinline__ int gmm_params2(MaskShared& S, const double* comp1, int init, int64_t n) {
    const int k = (int)(threadIdx.x & 1u);
    const double eps10 = 10.0 * DBL_EPSILON;
    double a[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) a[i] = k == 1 ? comp1[i] : S.tot[i] - comp1[i];
    const double nk = a[0] + eps10;
    double d[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double mu = (a[0] * S.mean[i] + a[1 + i]) / nk;
        d[i] = mu - S.mean[i];
    }
    double C[36];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            double v = a[7 + up(i, j)] - a[1 + i] * d[j] - d[i] * a[1 + j] + a[0] * d[i] * d[j];
            v = v / nk;
            C[i * 6 + j] = v; C[j * 6 + i] = v;
        }
#pragma unroll
    for (int i = 0; i < 6; ++i) C[i * 6 + i] += 1e-6;
    double U[21], ld;
    const int rc = prec_chol6_r(C, U, ld);
    // em_diff_form, per component: P_k = U_k U_k', m_k = mu_k - s (= d), P_k m_k, m_k' P_k m_k
    double P[36];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) {
            double v = 0.0;
#pragma unroll
            for (int j = c; j < 6; ++j) v += U[up(r, j)] * U[up(c, j)];
            P[r * 6 + c] = v; P[c * 6 + r] = v;
        }
    double q = 0.0, Pm[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double v = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) v += P[r * 6 + c] * d[c];
        Pm[r] = v;
        q += d[r] * v;
    }
    S.hnk[k] = nk; S.hq[k] = q; S.hrc[k] = rc;
    __builtin_amdgcn_wave_barrier();
    const bool ok = S.hrc[0] == 0 && S.hrc[1] == 0;
    if (ok) {                                   // both lanes: their component's parameters
        S.logdet[k] = ld;
        double* Pk = k ? S.L : S.C;             // P1 / P0 as em_diff_form keeps them
#pragma unroll
        for (int i = 0; i < 36; ++i) Pk[i] = P[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) S.hpm[6 * k + i] = Pm[i];
    }
    __builtin_amdgcn_wave_barrier();
    if (k != 0) return 0;
    if (!ok) return -1;
    // lane 0: weights, then the difference form from both components
    const double nk0 = S.hnk[0], nk1 = S.hnk[1];
    double w0, w1;
    if (init) { w0 = nk0 / (double)n; w1 = nk1 / (double)n; }
    else { const double sw = nk0 + nk1; w0 = nk0 / sw; w1 = nk1 / sw; }
    S.logw[0] = log(w0); S.logw[1] = log(w1);
    const double* P0 = S.C;
    const double* P1 = S.L;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = r; c < 6; ++c) {
            const double A = -0.5 * (P1[r * 6 + c] - P0[r * 6 + c]);
            S.Aq[up(r, c)] = r == c ? A : 2.0 * A;
        }
        S.bq[r] = S.hpm[6 + r] - S.hpm[r];
    }
    S.cq = -0.5 * (S.hq[1] - S.hq[0]) + (S.logdet[1] + S.logw[1]) - (S.logdet[0] + S.logw[0]);
    const double N = S.tot[0];
    double tr = 0.0, lin = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        lin += S.hpm[r] * S.tot[1 + r];
#pragma unroll
        for (int c = 0; c < 6; ++c) tr += P0[r * 6 + c] * S.tot[7 + (r <= c ? up(r, c) : up(c, r))];
    }
    const double K0 = -3.0 * log(2.0 * kPi) + S.logdet[0] + S.logw[0];
    S.C0 = N * K0 - 0.5 * (tr - 2.0 * lin + N * S.hq[0]);
    return 0;
}

// delta = v'A v + b'v + c (em_diff_form) for two points at once: every Aq / bq read from LDS
// serves both.
template <class Ptr>
SSF_DEV void em_delta2(const double va[6], const double vb[6], Ptr Aq, Ptr bq, double cq,
                       double& da, double& db) {
    da = cq; db = cq;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double ta = bq[j], tb = ta;
#pragma unroll
        for (int k = j; k < 6; ++k) { const double a = Aq[up(j, k)]; ta += a * va[k]; tb += a * vb[k]; }
        da += va[j] * ta; db += vb[j] * tb;
    }
}

template <class Ptr>
SSF_DEV double em_delta1(const double v[6], Ptr Aq, Ptr bq, double cq) {
    double d = cq;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double t = bq[j];
#pragma unroll
        for (int k = j; k < 6; ++k) t += Aq[up(j, k)] * v[k];
        d += v[j] * t;
    }
    return d;
}

// 1/d for d in [1, 2] (d = 1 + e, e in (0, 1]): v_rcp_f64 and two Newton steps, ~1 ulp,
// instead of the IEEE division sequence.
SSF_DEV double recip_1_2(double d) {
    double r = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-d, r, 1.0);
    return __builtin_fma(r, e, r);
}

}  // namespace ssf
