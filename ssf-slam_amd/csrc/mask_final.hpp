// mask_final.hpp -- the last stages of k_mask_pose: the final labels with the Kabsch sums and the
// published pose, the mask's flip pass, and the mode that takes the mask as given.
#pragma once
#include "mask_exchange.hpp"
#include "mask_gmm.hpp"
#include "mask_kabsch.hpp"

namespace ssf {

// ---- final E-step labels + label-1 Kabsch sums (label 0 = totals from pass 0 - label 1).
//      The mask is written in the same pass against a predicted background label (the
//      heavier component); the rare frame whose majority disagrees gets one flip pass.
// Reads the parameters, S.x0, ktot and the fit's counters; part 0 publishes the frame's out;
// writes S.bg and S.bg_pred for mask_flip.
template <class T>
SSF_DEV bool mask_final(MaskCtx<T>& C, const MaskLds& L, int reflection, uint8_t* __restrict__ bg_mask) {
    MaskShared& S = L.S;
    const int tid = threadIdx.x;
    const T* P = C.P;
    const T* Fl = C.Fl;
    const double (&mean)[6] = C.mean;
    const int64_t fb = C.fb, n = C.n, r0 = C.X.r0, r1 = C.X.r1;
    const int g = C.X.g;
    double* out = C.out;
    const int pred = S.logw[1] > S.logw[0] ? 1 : 0;
    const double cq = uni(S.cq);
    double x0[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) x0[d] = uni(S.x0[d]);
    double k1[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) k1[i] = 0.0;
    if (tid == 0) S.label0 = 0;
    __syncthreads();
    for_points_deep<kLloydDeep>(P, Fl, r0, r1, [&](int64_t i, const double* x, bool val) {
        // Aq / bq are re-read from LDS (broadcast ds_reads) for every point (lds_laundered)
        const LdsDouble* Aq = lds_laundered(S.Aq);
        const LdsDouble* bq = lds_laundered(S.bq);
        double v[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) v[a] = x[a] - mean[a];
        const int l = em_delta1(v, Aq, bq, cq) > 0.0 ? 1 : 0;   // a1 > a0
        // a slot past r1 holds point r1 - 1 again: its byte is rewritten with the same value
        if (bg_mask) bg_mask[fb + (val ? i : r1 - 1)] = (uint8_t)(l == pred);
        if (i == 0) S.label0 = l;
        const double w1 = val ? (double)l : 0.0;
        double sv[3], dv[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) { dv[r] = x[3 + r] - x0[3 + r]; sv[r] = dv[r] + (x[r] - x0[r]); }
        k1[0] += w1;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double ws = w1 * sv[r];
            k1[1 + r] += ws;
            k1[4 + r] += w1 * dv[r];
#pragma unroll
            for (int c = 0; c < 3; ++c) k1[7 + r * 3 + c] += ws * dv[c];
        }
    });
    block_sum_rs<16>(k1, L.red);
    if (C.X.G > 1) {                         // + the label of point 0 (part 0 has it)
        double v[17];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = k1[k];
        v[16] = g == 0 ? (double)S.label0 : 0.0;
        if (!exchange<17>(C.X, v, L.xtmp, &L.okflag)) return false;
#pragma unroll
        for (int k = 0; k < 16; ++k) k1[k] = v[k];
        if (tid == 0) S.label0 = (int)v[16];
        __syncthreads();
    }
    if (tid == 0) {
        S.passes += 1;
        const double n1 = k1[0];
        int bg;
        if (n1 * 2.0 > (double)n) bg = 1;
        else if (n1 * 2.0 < (double)n) bg = 0;
        else bg = S.label0;                     // Counter.most_common tie -> first seen
        S.bg = bg;
        S.bg_pred = pred;
        if (g == 0) {                           // part 0 publishes the frame's pose
            for (int i = 0; i < 26; ++i) out[i] = 0.0;
            double* kb = S.sums;
            for (int i = 0; i < 16; ++i) kb[i] = bg ? k1[i] : S.ktot[i] - k1[i];
            const double cs[3] = {S.x0[3] + S.x0[0], S.x0[4] + S.x0[1], S.x0[5] + S.x0[2]};
            const double cd[3] = {S.x0[3], S.x0[4], S.x0[5]};
            int st = S.status;
            if (st == 0) st = kabsch_finish(kb, cs, cd, reflection, out);
            out[SSF_POSE_OUT_STATUS] = st;
            out[SSF_POSE_OUT_BGLABEL] = bg;
            out[SSF_POSE_OUT_NBG] = kb[0];
            out[SSF_POSE_OUT_KM_ITER] = S.km_iter;
            out[SSF_POSE_OUT_EM_ITER] = S.em_iter;
            out[SSF_POSE_OUT_CONVERGED] = S.converged;
            out[SSF_POSE_OUT_CENTER0] = (double)S.c0;
            out[SSF_POSE_OUT_CENTER1] = (double)S.c1;
#ifdef SSF_MASK_STAMPS
            out[SSF_POSE_OUT_CENTER0] = S.dg_n > 0.0 ? S.dg_cyc / S.dg_n : 0.0;
            out[SSF_POSE_OUT_CENTER1] = S.dg_n > 0.0 ? S.dg_lab / (S.dg_n * (double)n) : 0.0;
            out[SSF_POSE_OUT_CONVERGED] = S.dg_wfull;
            out[SSF_POSE_OUT_NBG] = S.dg_full1;
            // EM pass split: points + block sum, exchange, M-step (cycles per pass)
            for (int k = 0; k < 3; ++k) out[SSF_POSE_OUT_T + k] = S.em_iter > 0 ? S.dg_e[k] / S.em_iter : 0.0;
#endif
            out[SSF_POSE_OUT_LOWER_BOUND] = S.lb;
            out[SSF_POSE_OUT_PASSES] = S.passes;
        }
    }
    __syncthreads();
    return true;
}

// The flip pass: the final pass wrote the mask against the predicted background label; where the
// majority label is the other one, the part's bytes are inverted.
template <class T>
SSF_DEV void mask_flip(const MaskCtx<T>& C, const MaskLds& L, uint8_t* __restrict__ bg_mask) {
    const MaskShared& S = L.S;
    const int tid = threadIdx.x;
    const int64_t fb = C.fb, r0 = C.X.r0, r1 = C.X.r1;
    if (bg_mask && S.bg != S.bg_pred) {
        for (int64_t i = r0 + tid; i < r1; i += blockDim.x) bg_mask[fb + i] ^= 1;
    }
}

// mode SSF_MASK_GT / SSF_MASK_GIVEN: background from the given / ground-truth mask; Kabsch sums
// shifted by point 0.  One work-group per frame, no fit.
template <class T>
SSF_DEV void mask_given(const MaskCtx<T>& C, const MaskLds& L, int mode, const uint8_t* __restrict__ mask_in,
                        int reflection, uint8_t* __restrict__ bg_mask) {
    MaskShared& S = L.S;
    const int tid = threadIdx.x;
    const T* P = C.P;
    const T* Fl = C.Fl;
    const int64_t fb = C.fb, n = C.n;
    double* out = C.out;
    double cs[3] = {0, 0, 0}, cd[3] = {0, 0, 0};
    if (n > 0) {
        double x0[6];
        load_x(P, Fl, 0, x0);
        for (int i = 0; i < 3; ++i) { cd[i] = x0[3 + i]; cs[i] = x0[3 + i] + x0[i]; }
    }
    double k[16];
    for (int i = 0; i < 16; ++i) k[i] = 0.0;
    for (int64_t i = tid; i < n; i += blockDim.x) {
        const uint8_t mv = mask_in[fb + i];
        const bool bg = (mode == SSF_MASK_GT) ? (mv == 0) : (mv != 0);
        if (bg_mask) bg_mask[fb + i] = bg ? 1 : 0;
        if (!bg) continue;
        double x[6];
        load_x(P, Fl, i, x);
        accum_kabsch(k, x, cs, cd);
    }
    block_sum_rs<16>(k, L.red);
    if (tid == 0) {
        for (int i = 0; i < SSF_POSE_OUT_STRIDE; ++i) out[i] = 0.0;
        for (int i = 0; i < 16; ++i) S.sums[i] = k[i];
        const int st = kabsch_finish(S.sums, cs, cd, reflection, out);
        out[SSF_POSE_OUT_STATUS] = st;
        out[SSF_POSE_OUT_BGLABEL] = -1;
        out[SSF_POSE_OUT_PASSES] = 1;
    }
}

}  // namespace ssf
