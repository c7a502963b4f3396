// mask_lloyd.hpp -- the Lloyd stage of the GMM fit of k_mask_pose: full passes, then passes that
// re-read only the points whose label could change.
#pragma once
#include "mask_exchange.hpp"

namespace ssf {

// The launch's record / queue buffer (mask_rec_bytes, lloyd_rec_count in ssf_internal.hpp).
// Records at an even offset (16-byte aligned pairs) with at least one spare slot (index n) after
// each frame: frame f's at ((fb + kLloydSpareRecs f + 1) & ~1).
SSF_DEV uint2* lloyd_rec_base(uint2* rec, int64_t fb, int f) {
    return rec + ((fb + kLloydSpareRecs * (int64_t)f + 1) & ~(int64_t)1);
}
// The relabel queues follow the records: frame f's at fb + kLloydSpareQueue f, n entries and the
// spare slots.
SSF_DEV uint32_t* lloyd_queue_base(uint2* rec, int64_t total, int n_frames, int64_t fb, int f) {
    return reinterpret_cast<uint32_t*>(rec + lloyd_rec_count(total, n_frames)) + fb + kLloydSpareQueue * (int64_t)f;
}

// ---- the lane-0 algebra around one Lloyd labelling pass, shared by iteration 0 (labelled in
//      the k-means++ candidate stream, mask_seed.hpp) and the loop of mask_lloyd.
// Lane 0, before the fit's first labelling pass.
SSF_DEV void lloyd_reset(MaskShared& S) {
    S.strict = 0; S.done = 0; S.lfull = 1;
    S.dg_cyc = S.dg_n = S.dg_lab = S.dg_wfull = S.dg_full1 = 0.0;
}
// Lane 0, before labelling pass `it`: the centres' squared norms S.csn and the pass's lhist row.
SSF_DEV void lloyd_begin_pass(MaskShared& S, int it) {
    double* h = S.lhist + 9 * it;
    for (int k = 0; k < 2; ++k) {
        double sn = 0.0;
        for (int d = 0; d < 6; ++d) sn += S.cen[6 * k + d] * S.cen[6 * k + d];
        S.csn[k] = sn;
    }
    for (int d = 0; d < 6; ++d) h[d] = S.cen[6 + d] - S.cen[d];
    h[6] = S.csn[0] - S.csn[1];
    h[7] = sqrt(S.csn[0]) + sqrt(S.csn[1]);
    h[8] = S.csn[0] + S.csn[1];
}
// Lane 0, after labelling pass `it`: acc = the pass's 14 cluster sums (full) or sum deltas (skip
// pass), changed / nlab = the frame's changed-label and relabelled counts, cost = the pass's
// traffic in 24-byte-per-point units.  Writes lsum, km_iter, lfull, passes, cenp / csnp, the new
// centres (an empty cluster keeps its centre), and strict / done from changed and the shift.
SSF_DEV void lloyd_end_pass(MaskShared& S, int it, bool full, const double (&acc)[14], int changed, int nlab,
                            int64_t n, double cost) {
    S.passes += cost;
    S.km_iter = it + 1;
    for (int k = 0; k < 14; ++k) S.lsum[k] = full ? acc[k] : S.lsum[k] + acc[k];
    // the first passes move the centres most (typically 35-45 % of the points would be
    // relabelled): full passes through it = 3, then skip passes while they relabel < 1/4
    S.lfull = full ? it < kLloydFullPasses - 1 : nlab * kLloydRefull > n;
    for (int k = 0; k < 12; ++k) S.cenp[k] = S.cen[k];
    S.csnp[0] = S.csn[0]; S.csnp[1] = S.csn[1];
    double shift = 0.0;
    for (int k = 0; k < 2; ++k) {
        const double wgt = S.lsum[7 * k];
        double sh = 0.0;
        for (int d = 0; d < 6; ++d) {
            const double nc = wgt > 0.0 ? S.lsum[7 * k + 1 + d] * (1.0 / wgt) : S.cen[6 * k + d];
            const double df = nc - S.cen[6 * k + d];
            sh += df * df;
            S.cen[6 * k + d] = nc;
        }
        sh = sqrt(sh);
        shift += sh * sh;
    }
    if (changed == 0) { S.strict = 1; S.done = 1; }
    else if (shift <= S.tol) S.done = 1;
}

// ---- Lloyd iterations (_kmeans_single_lloyd, max_iter 300) with exact label skipping.
//      A point's label at pass t is the sign of g_t = D0 - D1 (D_k = -2 v.c_k + |c_k|^2, the
//      expression the label is computed with).  In exact arithmetic g_t(v) = 2 v.w_t + s_t
//      (w = c1 - c0, s = |c0|^2 - |c1|^2), so |g_t - g_r| <= 2|v| |w_t - w_r| + |s_t - s_r|.
//      Every labelled point leaves an 8-byte record {|g_r| rounded down, |v| rounded up,
//      pass r, label}; a later pass t re-reads the point's 24 bytes only when
//          |g_r| <= B1(t, r) |v| + B2(t, r)
//      (B1/B2: the drift bounds plus 1e-13-relative margins for the f64 rounding of both
//      evaluations, >= 50x the dot-product error bound), i.e. whenever the sign could
//      differ.  Skipped points keep their label, so the labels, the changed-label count and
//      the strict-convergence decision are those of the full pass; the cluster sums are
//      updated by the points that changed label.
//      Iteration 0 (every point, against the k-means++ centres, no records) is not run here:
//      mask_kmeanspp labels it in its candidate stream and ends it with lloyd_end_pass.
// Reads iteration 0's result (S.cen, cenp / csnp, lsum, lfull, done, km_iter = 1) and S.tol;
// leaves the final centres in S.cen, the last labelling pass's in S.cenp / csnp, and S.strict,
// km_iter, passes.
// lloyd_rec: the launch's record / queue buffer; total: the points of all n_frames frames.
template <class T>
SSF_DEV bool mask_lloyd(MaskCtx<T>& C, const MaskLds& L, uint2* __restrict__ lloyd_rec, int64_t total,
                        int n_frames) {
    MaskShared& S = L.S;
    const int tid = threadIdx.x;
    const T* P = C.P;
    const T* Fl = C.Fl;
    const double (&mean)[6] = C.mean;
    const int64_t n = C.n, r0 = C.X.r0, r1 = C.X.r1;
    static_assert(kLloydFullPasses >= 2, "iteration 0 (mask_kmeanspp) writes no records");
    if (S.done) return true;                  // uniform: iteration 0 met tol (or no label changed)
    uint2* __restrict__ LR = lloyd_rec_base(lloyd_rec, C.fb, C.f);
    uint32_t* __restrict__ LQ = lloyd_queue_base(lloyd_rec, total, n_frames, C.fb, C.f);
    for (int it = 1; it < kLloydMax; ++it) {
        if (tid == 0) lloyd_begin_pass(S, it);
        __syncthreads();
        if (tid < it) {   // drift bounds of this pass against every earlier labelling pass
            const double* h = S.lhist + 9 * it;
            const double* g = S.lhist + 9 * tid;
            double dw = 0.0;
            for (int d = 0; d < 6; ++d) dw += (h[d] - g[d]) * (h[d] - g[d]);
            S.lb1[tid] = __double2float_ru(2.0 * sqrt(dw) + 2e-13 * (h[7] + g[7]));
            S.lb2[tid] = __double2float_ru(fabs(h[6] - g[6]) + 1e-13 * (h[8] + g[8]));
        }
        __syncthreads();
        // the centres are read from LDS (broadcast) at every point through a laundered base,
        // like the EM parameters: held in registers they spilled to scratch in these loops
        const double csn0 = uni(S.csn[0]), csn1 = uni(S.csn[1]);
        double acc[14];
#pragma unroll
        for (int k = 0; k < 14; ++k) acc[k] = 0.0;
        int changed = 0, nlab = 0;
        const bool full = S.lfull != 0;
#ifdef SSF_MASK_STAMPS
        const unsigned long long pass_t0 = __builtin_amdgcn_s_memtime();
#endif
        const bool wrec = it >= kLloydFullPasses - 1;   // a skip pass may follow this full pass
        // exact labelling of one point (the expression of every earlier version of this pass):
        // sums (full pass) or sum deltas (skip pass), changed count, new record
        // (val = 0: a pipeline slot with no point -- computed, weighted out, record written to
        // the frame's spare slot n)
        auto label = [&](auto wrec_c, int64_t i, const double* x, int lp, bool val) {
            const LdsDouble* cen = lds_laundered(S.cen);
            double v[6], dt0 = 0.0, dt1 = 0.0, vn = 0.0;
#pragma unroll
            for (int d = 0; d < 6; ++d) {
                v[d] = x[d] - mean[d];
                dt0 += v[d] * cen[d]; dt1 += v[d] * cen[6 + d]; vn += v[d] * v[d];
            }
            const double D0 = -2.0 * dt0 + csn0, D1 = -2.0 * dt1 + csn1;
            const int l = D1 < D0 ? 1 : 0;
            double d1 = full ? (double)l : (double)(l - lp), d0 = full ? 1.0 - d1 : -d1;
            d1 = val ? d1 : 0.0; d0 = val ? d0 : 0.0;
            changed += val && (it == 0 || l != lp);
            acc[0] += d0; acc[7] += d1;
#pragma unroll
            for (int d = 0; d < 6; ++d) { acc[1 + d] += d0 * v[d]; acc[8 + d] += d1 * v[d]; }
            // |g| one f32 ulp below its nearest float (<= |g|); |v| from an f32 sqrt, 4 ulps up,
            // then up to the 2^-14-relative grid that leaves the low 9 bits for the pass index
            const uint32_t gb = __float_as_uint((float)fabs(D0 - D1));
            const uint32_t nvb = (__float_as_uint(__builtin_sqrtf((float)vn)) + 4u + 0x1FFu) & 0x7FFFFE00u;
            if constexpr (decltype(wrec_c)::value) LR[val ? i : n] = make_uint2(gb ? gb - 1u : 0u, nvb | (uint32_t)it | ((uint32_t)l << 31));
        };
        if (full) {
            // every point: a prefetched stream of [flow, xyz]; the previous label is recomputed
            // from the previous centres (the pass that wrote it used the same expression)
            const double cpn0 = uni(S.csnp[0]), cpn1 = uni(S.csnp[1]);
            auto full_pass = [&](auto wrec_c) {
                for_points_deep<kLloydDeep>(P, Fl, r0, r1, [&](int64_t i, const double* x, bool val) {
                    const LdsDouble* cenp = lds_laundered(S.cenp);
                    double dp0 = 0.0, dp1 = 0.0;
#pragma unroll
                    for (int d = 0; d < 6; ++d) {
                        const double v = x[d] - mean[d];
                        dp0 += v * cenp[d]; dp1 += v * cenp[6 + d];
                    }
                    const int lp = (-2.0 * dp1 + cpn1) < (-2.0 * dp0 + cpn0) ? 1 : 0;
                    label(wrec_c, i, x, lp, val);
                });
            };
            if (wrec) full_pass(std::true_type{});    // two loop bodies: no branch per point
            else full_pass(std::false_type{});
            nlab = (int)((r1 - r0 - tid + blockDim.x - 1) / blockDim.x);
        } else {
            // skip pass, two streams per wave over its own segment.  (1) the records, 16 bytes
            // (two records) per lane per load, 8 loads in flight: the points whose sign could
            // change are appended (ballot compaction, label in bit 31) to the wave's queue in
            // global memory.  (2) the queue, 512 entries at a time: every entry load, then every
            // point gather, then the relabelling -- two round trips per 512 queued points.
            const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = lane_id();
            const int64_t seg = ((r1 - r0 + kNW - 1) / kNW + 127) / 128 * 128;
            const int64_t ws = r0 + (int64_t)w * seg, we = ws + seg < r1 ? ws + seg : r1;
            uint32_t* __restrict__ WQ = LQ + ws;        // capacity seg >= the wave's points
            const int64_t qspare = n - ws;               // LQ[n, n + 64): spare slots
            const uint4* __restrict__ LR4 = reinterpret_cast<const uint4*>(LR);
            const int64_t plast = (n - 1) >> 1;
            uint32_t* Q = L.lq + w * kLQ;               // this trip's entries (<= D * 128)
            int qc = 0, nl = 0;                         // wave-uniform
            constexpr int D = kLloydRecDeep;
            uint4 buf[D];
#pragma unroll
            for (int d = 0; d < D; ++d) buf[d] = LR4[min((ws >> 1) + d * 64 + lane, plast)];
            for (int64_t base = ws; base < we; base += D * 128) {
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const int64_t b = base + d * 128;
                    const uint4 q = buf[d];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const uint32_t gx = h ? q.z : q.x, gy = h ? q.w : q.y;
                        const int64_t i = b + 2 * lane + h;
                        const int tr = (int)(gy & 0x1FFu);
                        const float nv = __uint_as_float(gy & 0x7FFFFE00u);
                        const bool skip = __uint_as_float(gx) > __builtin_fmaf(S.lb1[tr], nv, S.lb2[tr]) * 1.00001f;
                        const bool nd = (i < we) & !skip;
                        const uint64_t m = __ballot(nd);
                        if (nd) Q[nl + __popcll(m & lanemask_lt())] = (uint32_t)i | (gy & 0x80000000u);
                        nl += __popcll(m);
                    }
                    // reloaded only after q is consumed: the load can reuse q's registers, so
                    // the loop-carried buffers need no copies (a copy waits for its load)
                    buf[d] = LR4[min(((b + D * 128) >> 1) + lane, plast)];
                }
                // the trip's queue entries leave LDS: two unconditional 64-entry stores (lanes
                // without an entry write the frame's spare slots), more only past 128 entries
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    WQ[h * 64 + lane < nl ? qc + h * 64 + lane : qspare + lane] = Q[h * 64 + lane];
                for (int k = 128; k < nl; k += 64)
                    if (k + lane < nl) WQ[qc + k + lane] = Q[k + lane];
                __builtin_amdgcn_wave_barrier();
                qc += nl;
                nl = 0;
            }
            __threadfence_block();   // the wave's queue stores are visible to its loads below
            for (int j0 = 0; j0 < qc; j0 += 512) {
                uint32_t e[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) e[k] = WQ[min(j0 + k * 64 + lane, qc - 1)];
                T px[8][6];
#pragma unroll
                for (int k = 0; k < 8; ++k) load_raw(P, Fl, (int64_t)(e[k] & 0x7FFFFFFFu), px[k]);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    double x[6];
#pragma unroll
                    for (int d = 0; d < 6; ++d) x[d] = (double)px[k][d];
                    const bool val = j0 + k * 64 + lane < qc;
                    label(std::true_type{}, (int64_t)(e[k] & 0x7FFFFFFFu), x, (int)(e[k] >> 31), val);
                    nlab += val ? 1 : 0;
                }
            }
        }
        block_sum_rs<14>(acc, L.red);
        changed = block_sum_scalar<int>(changed, L.ired);
        nlab = block_sum_scalar<int>(nlab, L.ired);
        if (C.X.G > 1) {
            double v[16];
#pragma unroll
            for (int k = 0; k < 14; ++k) v[k] = acc[k];
            v[14] = (double)changed; v[15] = (double)nlab;
            if (!exchange<16>(C.X, v, L.xtmp, &L.okflag)) return false;
#pragma unroll
            for (int k = 0; k < 14; ++k) acc[k] = v[k];
            changed = (int)v[14]; nlab = (int)v[15];
        }
        if (tid == 0) {
            // traffic accounting in 24-byte-per-point units: a full pass reads [flow, xyz] (+8 B
            // of records written when wrec); a skip pass reads 8 B of records per point and
            // 24 B per relabelled point, and writes (reads) 8 B of record + 4 (4) B of queue
            // per relabel
            lloyd_end_pass(S, it, full, acc, changed, nlab, n,
                           full ? 1.0 + (wrec ? 8.0 / 24.0 : 0.0)
                                : (8.0 * (double)n + 40.0 * (double)nlab) / (24.0 * (double)n));
#ifdef SSF_MASK_STAMPS
            // diagnostic: cycles and relabelled points of the skip passes (k_mask_pose stamps
            // build only; reported through the k-means++ centre slots, which it overwrites)
            if (!full) { S.dg_cyc += (double)(__builtin_amdgcn_s_memtime() - pass_t0); S.dg_n += 1.0; S.dg_lab += nlab; }
            else if (it == kLloydFullPasses - 1) S.dg_wfull = (double)(__builtin_amdgcn_s_memtime() - pass_t0);
            else if (it == 1) S.dg_full1 = (double)(__builtin_amdgcn_s_memtime() - pass_t0);
#endif
        }
        __syncthreads();
        if (S.done) break;
    }
    return true;
}

}  // namespace ssf
