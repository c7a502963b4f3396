// mask_em.hpp -- the GMM stages of k_mask_pose: the initial parameters from the k-means labels,
// then EM, one fused E-step + M-step pass per iteration.
#pragma once
#include "mask_exchange.hpp"
#include "mask_gmm.hpp"

namespace ssf {

// ---- GMM init from one-hot k-means labels: strict convergence keeps the labels of the last
//      pass (centres S.cenp), otherwise sklearn relabels with the final centres (S.cen).
//      Only cluster 1's moments are summed, cluster 0 = total - cluster 1.
// Writes the first parameters (gmm_params2: S.Aq, bq, cq, C0, logw, logdet), S.lb, done, status.
// mstep(init): the kernel's call of gmm_params2 on S.sums.  It is handed in because gmm_params2
// is not inlined: only a call that names the LDS variable itself lets the compiler fold the
// addresses of S into gmm_params2's body (a third fewer LDS instructions there).
template <class T, class MStep>
SSF_DEV bool mask_gmm_init(MaskCtx<T>& C, const MaskLds& L, MStep&& mstep) {
    MaskShared& S = L.S;
    const int tid = threadIdx.x;
    const T* P = C.P;
    const T* Fl = C.Fl;
    const double (&mean)[6] = C.mean;
    const int64_t r0 = C.X.r0, r1 = C.X.r1;
    double cen[12], csn0, csn1;
    if (S.strict) {
#pragma unroll
        for (int k = 0; k < 12; ++k) cen[k] = uni(S.cenp[k]);
        csn0 = S.csnp[0]; csn1 = S.csnp[1];
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) cen[k] = uni(S.cen[k]);
        csn0 = 0.0; csn1 = 0.0;
        for (int d = 0; d < 6; ++d) { csn0 += cen[d] * cen[d]; csn1 += cen[6 + d] * cen[6 + d]; }
    }
    double acc[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = 0.0;
    for_points_deep<kLloydDeep>(P, Fl, r0, r1, [&](int64_t, const double* x, bool val) {
        double v[6], dt0 = 0.0, dt1 = 0.0;
#pragma unroll
        for (int d = 0; d < 6; ++d) { v[d] = x[d] - mean[d]; dt0 += v[d] * cen[d]; dt1 += v[d] * cen[6 + d]; }
        const int l = (-2.0 * dt1 + csn1) < (-2.0 * dt0 + csn0) ? 1 : 0;
        const double w1 = val ? (double)l : 0.0;
        acc[0] += w1;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const double wv = w1 * v[a];
            acc[1 + a] += wv;
#pragma unroll
            for (int b = a; b < 6; ++b) acc[7 + up(a, b)] += wv * v[b];
        }
    });
    block_sum_rs<28>(acc, L.red);
    if (!exchange<28>(C.X, acc, L.xtmp, &L.okflag)) return false;
    if (tid < 2) {                           // lanes 0 / 1: the two components
        if (tid == 0) {
            S.passes += 1;
            for (int k = 0; k < 28; ++k) S.sums[k] = acc[k];
        }
        const int rc = mstep(1);
        if (tid == 0) {
            if (rc != 0) S.status = SSF_POSE_GMM_FAILED;
            S.lb = -__builtin_inf();
            S.done = 0;
        }
    }
    __syncthreads();
    return true;
}

// ---- EM: one fused pass per iteration -- E-step with the current parameters and the
//      M-step moments of component 1 (component 0 = total - component 1), in the
//      difference form of em_diff_form: per point only delta = a1 - a0 (27 FMAs instead of
//      two 27-FMA Mahalanobis forms), e = exp(-|delta|), r1 = 1/(1+e) if delta > 0 else
//      e/(1+e), and the lower bound's per-point part max(delta, 0) + log1p(e).
// Reads and rewrites the parameters (mstep, see mask_gmm_init); writes S.lb, em_iter, converged,
// status.
template <class T, class MStep>
SSF_DEV bool mask_em(MaskCtx<T>& C, const MaskLds& L, MStep&& mstep) {
    MaskShared& S = L.S;
    const int tid = threadIdx.x;
    const T* P = C.P;
    const T* Fl = C.Fl;
    const double (&mean)[6] = C.mean;
    const int64_t n = C.n, r0 = C.X.r0, r1 = C.X.r1;
    for (int it = 1; it <= 100 && S.status == 0; ++it) {
        const double cq = uni(S.cq);
        double acc[29];
#pragma unroll
        for (int k = 0; k < 29; ++k) acc[k] = 0.0;
        // sum of log1p(e) over the thread's points = log of the product of (1 + e), kept as
        // mantissa * 2^pexp (frexp per pair: the product never overflows, one log per thread)
        double prod = 1.0;
        int pexp = 0;
#ifdef SSF_MASK_STAMPS
        if (it == 1 && tid == 0) S.dg_e[0] = S.dg_e[1] = S.dg_e[2] = 0.0;
        const unsigned long long e_t0 = __builtin_amdgcn_s_memtime();
#endif
        // the laundered LDS bases outside the loop: two loop-invariant VGPRs (the parameter
        // reads themselves stay in the loop, see the pair body).  Laundered per
        // pair, their constants were rematerialised every iteration into registers the
        // prefetched point loads had landed in, so the loads were copied away (and waited for)
        // right after they were issued
        const LdsDouble* AqL = lds_laundered(S.Aq);
        const LdsDouble* bqL = lds_laundered(S.bq);
        // one point's E-step from its delta and its M-step moments; returns d = 1 + e
        auto em_point = [&](const double* v, double dl) {
            const double e = exp(-fabs(dl));
            const double d = 1.0 + e;
            acc[28] += dl > 0.0 ? dl : 0.0;
            const double inv = recip_1_2(d);
            const double r = dl > 0.0 ? inv : e * inv;
            acc[0] += r;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double rv = r * v[a];
                acc[1 + a] += rv;
#pragma unroll
                for (int b = a; b < 6; ++b) acc[7 + up(a, b)] += rv * v[b];
            }
            return d;
        };
        // prod is in [0.5, 1) (1 at the start) and every d in (1, 2], so two factors stay below 4:
        // one renormalisation per pair, and a power-of-two scale commutes with the rounding
        auto renorm = [&]() {
            pexp += __builtin_amdgcn_frexp_exp(prod);
            prod = __builtin_amdgcn_frexp_mant(prod);
        };
        for_point_pairs(P, Fl, r0, r1, [&](const double* xa, const double* xb) {
            double va[6], vb[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) { va[a] = xa[a] - mean[a]; vb[a] = xb[a] - mean[a]; }
            double da, db;
            // the 27 parameters are read from LDS for every pair (the compiler may not keep them
            // across this point).  Held in VGPRs for the pass, as before the lone-point body
            // existed, they leave this loop short of registers: one parameter reloaded from
            // scratch per pair and the prefetched loads waited for in the iteration that issues
            // them (mask alone -5 %)
            asm volatile("" ::: "memory");
            em_delta2(va, vb, AqL, bqL, cq, da, db);
            prod *= em_point(va, da);
            prod *= em_point(vb, db);
            renorm();
        }, [&](const double* xa) {               // em_delta1: the operations of one half of em_delta2
            double va[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) va[a] = xa[a] - mean[a];
            prod *= em_point(va, em_delta1(va, AqL, bqL, cq));
            renorm();
        });
        acc[28] += log(prod) + (double)pexp * 0.69314718055994530942;
        block_sum_rs<29>(acc, L.red);
#ifdef SSF_MASK_STAMPS
        const unsigned long long e_t1 = __builtin_amdgcn_s_memtime();
#endif
        if (!exchange<29>(C.X, acc, L.xtmp, &L.okflag)) return false;
#ifdef SSF_MASK_STAMPS
        const unsigned long long e_t2 = __builtin_amdgcn_s_memtime();
#endif
        if (tid < 2) {                           // lanes 0 / 1: the two components
            double prev = 0.0;
            if (tid == 0) {
                S.passes += 1;
                S.em_iter = it;
                prev = S.lb;
                S.lb = (S.C0 + acc[28]) / (double)n;   // C0: the a0 part, from this E-step's parameters
                for (int k = 0; k < 29; ++k) S.sums[k] = acc[k];
            }
            const int rc = mstep(0);
            if (tid == 0) {
                if (rc != 0) S.status = SSF_POSE_GMM_FAILED;
                if (fabs(S.lb - prev) < 1e-3) { S.converged = 1; S.done = 1; }
            }
        }
        __syncthreads();
#ifdef SSF_MASK_STAMPS
        if (tid == 0) {
            S.dg_e[0] += (double)(e_t1 - e_t0); S.dg_e[1] += (double)(e_t2 - e_t1);
            S.dg_e[2] += (double)(__builtin_amdgcn_s_memtime() - e_t2);
        }
#endif
        if (S.done) break;
    }
    return true;
}

}  // namespace ssf
