// mask_seed.hpp -- the first two stages of the GMM fit of k_mask_pose: the pass-0 moments and
// the k-means++ seeding of the two Lloyd centres.  Two streams of the part do the work of four:
//   pass 0      the moments AND the distances to the first centre (the k-means++ block totals)
//   candidates  the two candidates' potentials AND Lloyd iteration 0 under either candidate
#pragma once
#include "mask_lloyd.hpp"

namespace ssf {

// D(i), the squared distance of point x to the first centre xc, both as stored: the mean is not
// needed (|v_i - v_c|^2 with v = x - mean), so pass 0 can form it before the mean exists.  The
// one expression of D everywhere it is needed (pass 0 or the first k-means++ stream, the re-scan
// of the draws' blocks, the candidate stream), so a recomputed D has the bits of the summed one.
SSF_DEV double dist0(const double* x, const double (&xc)[6]) {
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < 6; ++d) { const double u = x[d] - xc[d]; s += u * u; }
    return s;
}

// The first centre's index: the caller's draw, clamped (known before any point is read).
SSF_DEV int64_t first_centre(const double* __restrict__ draws, int f, int64_t n) {
    int64_t c0 = (int64_t)draws[3 * f];
    if (c0 < 0) c0 = 0;
    if (c0 >= n) c0 = n - 1;
    return c0;
}

// The k-means++ cumulative sum runs over 64-point blocks of the part; wave w owns the contiguous
// blocks [w spw, (w + 1) spw).  The block totals live in LDS (L.bsum) when they fit.
struct KppSeg {
    int64_t seg, spw;          // points / blocks per wave segment
    bool use_blocks;           // uniform
};
SSF_DEV KppSeg kpp_seg(int64_t nloc) {
    KppSeg k;
    const int nw = blockDim.x >> 6;
    k.seg = (((nloc + nw - 1) / nw) + 63) / 64 * 64;
    k.spw = k.seg / 64;
    k.use_blocks = k.spw * nw <= kKppBlocks;
    return k;
}

// the in-block inclusive scan of one value per lane (pass 0 / the first k-means++ stream and the
// re-scan of a draw's block: the same steps, so the same bits)
SSF_DEV double block_scan(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double y = __shfl_up(v, o, 64);
        if (lane >= o) v += y;
    }
    return v;
}

// ---- pass 0: column means, variances (KMeans tol) and the total first/second moments
//      about point 0, converted by lane 0 to moments about the mean (the common shift of
//      every later moment sum).  The same stream forms D(i) to the first centre and leaves the
//      in-order total of every 64-point block of the part in L.bsum (parts of at most
//      kKppBlocks blocks; mask_kmeanspp streams larger ones itself).
// Writes S.mean, tol, tot, x0, ktot, c0 (the first centre, from the caller's draw) and passes.
template <class T>
SSF_DEV bool mask_pass0(MaskCtx<T>& C, const MaskLds& L, const double* __restrict__ draws) {
    MaskShared& S = L.S;
    const int tid = threadIdx.x;
    const T* P = C.P;
    const T* Fl = C.Fl;
    const int64_t n = C.n, r0 = C.X.r0, r1 = C.X.r1;
    double x0[6], xc0[6];
    load_x(P, Fl, 0, x0);
    const int64_t c0 = first_centre(draws, C.f, n);
    load_x(P, Fl, c0, xc0);
    double a[27];
#pragma unroll
    for (int i = 0; i < 27; ++i) a[i] = 0.0;
    auto moments = [&](const double* x, bool val) {
        double v[6], vw[6];
#pragma unroll
        for (int d = 0; d < 6; ++d) { v[d] = x[d] - x0[d]; vw[d] = val ? v[d] : 0.0; a[d] += vw[d]; }
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) a[6 + up(r, c)] += vw[r] * v[c];
    };
    // two points in flight per thread (for_points_deep: the same per-thread order, so the
    // same sums); a slot past r1 adds zeros
    if (kpp_seg(r1 - r0).use_blocks) {
        // a wave's trips taken together: at slot j the wave holds block j >> 6 of the part, whose
        // inclusive scan's last value is the block's total (an empty slot's D is 0)
        const int lane = lane_id();
        const uint32_t nblk = (uint32_t)((r1 - r0 + 63) >> 6);   // <= kKppBlocks
        for_points_deep<kLloydDeep, true>(P, Fl, r0, r1, [&](int64_t i, const double* x, bool val) {
            moments(x, val);
            const double d = block_scan(val ? dist0(x, xc0) : 0.0, lane);
            const uint32_t blk = (uint32_t)(i - r0) >> 6;
            if (lane == 63 && blk < nblk) L.bsum[blk] = d;
        });
    } else {
        for_points_deep<kLloydDeep>(P, Fl, r0, r1, [&](int64_t, const double* x, bool val) { moments(x, val); });
    }
    block_sum_rs<27>(a, L.red);               // its barriers also publish bsum to the other waves
    if (!exchange<27>(C.X, a, L.xtmp, &L.okflag)) return false;
    if (tid == 0) {
        const double nn = (double)n;
        double m[6];
        double tol = 0.0;
        for (int d = 0; d < 6; ++d) { m[d] = a[d] / nn; S.mean[d] = x0[d] + m[d]; }
        S.tot[0] = nn;
        for (int d = 0; d < 6; ++d) S.tot[1 + d] = a[d] - nn * m[d];
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) S.tot[7 + up(r, c)] = a[6 + up(r, c)] - nn * m[r] * m[c];
        for (int d = 0; d < 6; ++d) tol += S.tot[7 + up(d, d)] / nn;
        S.tol = tol / 6.0 * 1e-4;
        // Kabsch sums over ALL points about (cs, cd) = (x0_p + x0_f, x0_p), from the raw
        // moments about x0: s - cs = v_f + v_p, d - cd = v_p  (v = x - x0; f = 0..2, p = 3..5)
        for (int d = 0; d < 6; ++d) S.x0[d] = x0[d];
        S.ktot[0] = nn;
        for (int r = 0; r < 3; ++r) { S.ktot[1 + r] = a[r] + a[3 + r]; S.ktot[4 + r] = a[3 + r]; }
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                const int fr = r, pr = 3 + r, pc = 3 + c;
                const double sfp = a[6 + (fr <= pc ? up(fr, pc) : up(pc, fr))];
                const double spp = a[6 + (pr <= pc ? up(pr, pc) : up(pc, pr))];
                S.ktot[7 + r * 3 + c] = sfp + spp;
            }
        S.c0 = c0;
        S.passes = 1;
    }
    __syncthreads();
    return true;
}

// ---- k-means++ (sklearn _kmeans_plusplus, n_local_trials = 2), ending in Lloyd iteration 0
// Reads S.c0, pass 0's block totals L.bsum and the caller's two draws; writes S.c1, the two
// centres and -- the candidate stream labels every point against (first centre, candidate j) for
// both candidates, and the winner's cluster sums are Lloyd iteration 0's -- everything that
// iteration leaves (lloyd_end_pass), and passes.
template <class T>
SSF_DEV bool mask_kmeanspp(MaskCtx<T>& C, const MaskLds& L, const double* __restrict__ draws) {
    MaskShared& S = L.S;
    const int tid = threadIdx.x;
    const T* P = C.P;
    const T* Fl = C.Fl;
    const double (&mean)[6] = C.mean;
    const int64_t n = C.n, r0 = C.X.r0, r1 = C.X.r1;
    const int f = C.f;
    double xc0[6], c0[6], cn0 = 0.0;
    load_x(P, Fl, S.c0, xc0);
    for (int d = 0; d < 6; ++d) { c0[d] = xc0[d] - mean[d]; cn0 += c0[d] * c0[d]; }
    // distances to the first centre; each wave owns a contiguous segment so the
    // in-order cumulative sum needs only one block-level exchange of wave totals
    const int nw = blockDim.x >> 6, w = tid >> 6, lane = lane_id();
    const KppSeg ks = kpp_seg(r1 - r0);
    const int64_t seg = ks.seg, spw = ks.spw;
    const bool use_blocks = ks.use_blocks;                   // uniform
    const int64_t ws = r0 + (int64_t)w * seg, we = ws + seg < r1 ? ws + seg : r1;
    // D(i) is recomputed (same expression, same bits) wherever it is needed instead of being stored
    auto dist0i = [&](int64_t i) {
        double x[6];
        load_x(P, Fl, i, x);
        return dist0(x, xc0);
    };
    constexpr int kKppDeep = SSF_KPP_DEEP;
    const int64_t wlast = we > ws ? we - 1 : ws;
    double wsum = 0.0;
    if (use_blocks) {
        // pass 0 left every block's total: the wave adds up its own blocks'
        for (int64_t k = lane; ws + 64 * k < we; k += 64) wsum += L.bsum[w * spw + k];
    } else {
        // a part above kKppBlocks blocks: the wave's segment streamed with the next kKppDeep
        // blocks' points in flight (raw floats, loads clamped and unconditional)
        T kb[kKppDeep][6];
        if (ws < we) {
#pragma unroll
            for (int k = 0; k < kKppDeep; ++k) load_raw_stream(P, Fl, min(ws + 64 * k + lane, wlast), kb[k]);
        }
        for (int64_t b0 = ws; b0 < we; b0 += 64 * kKppDeep)
#pragma unroll
        for (int k = 0; k < kKppDeep; ++k) {
            const int64_t b = b0 + 64 * k;
            if (b >= we) break;                              // uniform
            const int64_t i = b + lane;
            double x[6];
#pragma unroll
            for (int d = 0; d < 6; ++d) x[d] = (double)kb[k][d];
            load_raw_stream(P, Fl, min(i + 64 * kKppDeep, wlast), kb[k]);
            wsum += i < we ? dist0(x, xc0) : 0.0;
        }
        if (tid == 0) S.passes += 1;
    }
    wsum = wave_sum(wsum);
    if (lane == 0) L.red[w] = wsum;
    if (tid == 0) { L.cand[0] = (unsigned long long)n; L.cand[1] = (unsigned long long)n; }
    __syncthreads();
    double pot = 0.0, carry = 0.0;
    for (int k = 0; k < nw; ++k) { if (k == w) carry = pot; pot += L.red[k]; }
    if (C.X.G > 1) {
        // the in-order cumulative sum runs over the parts in order: part g starts after the
        // potentials of parts 0..g-1 (one value per part; every part reads all G in order)
        double before = 0.0, total = 0.0;
        if (!exchange_prefix(C.X, pot, L.xtmp, &L.okflag, before, total)) return false;
        carry += before;
        pot = total;
    }
    // the two draws on the cumulative potential
    const double t1 = draws[3 * f + 1] * pot, t2 = draws[3 * f + 2] * pot;
    // wave-local in-order inclusive scan of its segment; first index with cumsum >= rand.
    // A wave whose whole segment ends below both draws cannot hold either index and skips
    // the scan (1e-9 slack >> the scan's rounding); the others stop once both are found.
    const double wtot = L.red[w];
    bool f1 = carry + wtot < t1 * (1.0 - 1e-9), f2 = carry + wtot < t2 * (1.0 - 1e-9);
    if (use_blocks) {
        // walk the wave's block totals with the same carry arithmetic as the full scan
        // (carry + block total, then carry += total): the first block whose end reaches a
        // draw is the block the full scan would stop in; only that block is re-scanned
        int64_t blk1 = -1, blk2 = -1;
        double cb1 = 0.0, cb2 = 0.0;
        if (lane == 0 && !(f1 && f2)) {
            double cr = carry;
            for (int64_t k = 0; ws + 64 * k < we; ++k) {
                const double tot = L.bsum[w * spw + k];
                if (!f1 && blk1 < 0 && cr + tot >= t1) { blk1 = k; cb1 = cr; }
                if (!f2 && blk2 < 0 && cr + tot >= t2) { blk2 = k; cb2 = cr; }
                if ((f1 || blk1 >= 0) && (f2 || blk2 >= 0)) break;
                cr += tot;
            }
        }
        blk1 = __shfl(blk1, 0, 64); blk2 = __shfl(blk2, 0, 64);
        cb1 = __shfl(cb1, 0, 64); cb2 = __shfl(cb2, 0, 64);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t blk = j ? blk2 : blk1;
            if (blk < 0) continue;                           // wave-uniform
            const int64_t b = ws + 64 * blk;
            const int64_t i = b + lane;
            const double v = block_scan(i < we ? dist0i(i) : 0.0, lane);
            const double incl = (j ? cb2 : cb1) + v;
            const uint64_t mm = __ballot(i < we && incl >= (j ? t2 : t1));
            if (mm && lane == 0) atomicMin(&L.cand[j], (unsigned long long)(b + __ffsll((unsigned long long)mm) - 1));
        }
        f1 = f2 = true;                                      // skip the sequential scan
    } else if (tid == 0) {
        S.passes += 1;                                       // the sequential scan below
    }
    for (int64_t b = ws; b < we && !(f1 && f2); b += 64) {
        const int64_t i = b + lane;
        const double v = block_scan(i < we ? dist0i(i) : 0.0, lane);
        const double incl = carry + v;
        const uint64_t m1 = __ballot(i < we && incl >= t1), m2 = __ballot(i < we && incl >= t2);
        if (!f1 && m1) { f1 = true; if (lane == 0) atomicMin(&L.cand[0], (unsigned long long)(b + __ffsll((unsigned long long)m1) - 1)); }
        if (!f2 && m2) { f2 = true; if (lane == 0) atomicMin(&L.cand[1], (unsigned long long)(b + __ffsll((unsigned long long)m2) - 1)); }
        carry += __shfl(v, 63, 64);
    }
    __syncthreads();
    double cmin[2] = {(double)L.cand[0], (double)L.cand[1]};   // < 2^53: exact
    if (!exchange<2, true>(C.X, cmin, L.xtmp, &L.okflag)) return false;
    const int64_t cand[2] = {cmin[0] < (double)n ? (int64_t)cmin[0] : n - 1,
                             cmin[1] < (double)n ? (int64_t)cmin[1] : n - 1};
    double cc[2][6], ccn[2] = {0.0, 0.0};
    for (int j = 0; j < 2; ++j) {
        double x[6];
        load_x(P, Fl, cand[j], x);
        for (int d = 0; d < 6; ++d) { cc[j][d] = x[d] - mean[d]; ccn[j] += cc[j][d] * cc[j][d]; }
    }
    // The candidate stream, in the Lloyd full pass's per-thread order.  Per point the dots with
    // the first centre and the two candidates give each candidate's potential term min(D, D_j)
    // and, for hypothesis j = "candidate j wins", the label of Lloyd iteration 0 against
    // (c0, cand_j): the expression of mask_lloyd's label (D_k = -2 v.c_k + |c_k|^2), its 14 cluster
    // sums in the full-pass form.  s = {potentials [2], sums under j = 0 [14], under j = 1 [14]}.
    double s[30];
#pragma unroll
    for (int k = 0; k < 30; ++k) s[k] = 0.0;
    // 1.0 in SGPRs the optimiser cannot see through.  As a literal, the label's select shares one
    // VGPR pair holding 1.0 with mask_lloyd's loops; that pair then lives from the kernel's start,
    // is spilled, and was reloaded per point inside the Lloyd full pass (2.4 -> 3.4 10^5 cycles).
    int one_hi;
    asm volatile("s_mov_b32 %0, 0x3ff00000" : "=s"(one_hi));
    const double one = __hiloint2double(one_hi, 0);
    for_points_deep<kLloydDeep>(P, Fl, r0, r1, [&](int64_t, const double* x, bool val) {
        double v[6], dtc = 0.0, dt[2] = {0.0, 0.0}, xs = 0.0;
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            v[d] = x[d] - mean[d];
            dtc += v[d] * c0[d]; dt[0] += v[d] * cc[0][d]; dt[1] += v[d] * cc[1][d]; xs += v[d] * v[d];
        }
        const double di = dist0(x, xc0);
        const double D0 = -2.0 * dtc + cn0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double D1 = -2.0 * dt[j] + ccn[j];
            double vj = D1 + xs;
            vj = vj > 0.0 ? vj : 0.0;
            vj = vj < di ? vj : di;
            s[j] += val ? vj : 0.0;
            double d1 = D1 < D0 ? one : 0.0, d0 = 1.0 - d1;
            d1 = val ? d1 : 0.0; d0 = val ? d0 : 0.0;
            double* acc = s + 2 + 14 * j;
            acc[0] += d0; acc[7] += d1;
#pragma unroll
            for (int d = 0; d < 6; ++d) { acc[1 + d] += d0 * v[d]; acc[8 + d] += d1 * v[d]; }
        }
    });
    block_sum_rs<30>(s, L.red);
    if (!exchange<30>(C.X, s, L.xtmp, &L.okflag)) return false;
    const bool best = s[1] < s[0];                           // uniform: every thread holds the totals
    double acc[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) acc[k] = best ? s[16 + k] : s[2 + k];
    if (tid == 0) {
        S.c1 = cand[best ? 1 : 0];
        for (int d = 0; d < 6; ++d) { S.cen[d] = c0[d]; S.cen[6 + d] = best ? cc[1][d] : cc[0][d]; }
        for (int d = 0; d < 12; ++d) S.cenp[d] = 0.0;
        S.csnp[0] = S.csnp[1] = 0.0;
        // Lloyd iteration 0 is done: every label is new (changed = n, never strict), no records;
        // the stream counts once for both
        lloyd_reset(S);
        lloyd_begin_pass(S, 0);
        lloyd_end_pass(S, 0, true, acc, n > 0x7fffffff ? 0x7fffffff : (int)n, 0, n, 1.0);
    }
    __syncthreads();
    return true;
}

}  // namespace ssf
