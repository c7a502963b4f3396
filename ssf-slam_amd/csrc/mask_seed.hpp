// mask_seed.hpp -- the first two stages of the GMM fit of k_mask_pose: the pass-0 moments and
// the k-means++ seeding of the two Lloyd centres.
#pragma once
#include "mask_exchange.hpp"

namespace ssf {

// ---- pass 0: column means, variances (KMeans tol) and the total first/second moments
//      about point 0, converted by lane 0 to moments about the mean (the common shift of
//      every later moment sum).
// Writes S.mean, tol, tot, x0, ktot, c0 (the first centre, from the caller's draw) and passes.
template <class T>
SSF_DEV bool mask_pass0(MaskCtx<T>& C, const MaskLds& L, const double* __restrict__ draws) {
    MaskShared& S = L.S;
    const int tid = threadIdx.x;
    const T* P = C.P;
    const T* Fl = C.Fl;
    const int64_t n = C.n, r0 = C.X.r0, r1 = C.X.r1;
    double x0[6];
    load_x(P, Fl, 0, x0);
    double a[27];
#pragma unroll
    for (int i = 0; i < 27; ++i) a[i] = 0.0;
    // two points in flight per thread (for_points_deep: the same per-thread order, so the
    // same sums); a slot past r1 adds zeros
    for_points_deep<kLloydDeep>(P, Fl, r0, r1, [&](int64_t, const double* x, bool val) {
        double v[6], vw[6];
#pragma unroll
        for (int d = 0; d < 6; ++d) { v[d] = x[d] - x0[d]; vw[d] = val ? v[d] : 0.0; a[d] += vw[d]; }
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) a[6 + up(r, c)] += vw[r] * v[c];
    });
    block_sum_rs<27>(a, L.red);
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
        S.c0 = (int64_t)draws[3 * C.f];
        if (S.c0 < 0) S.c0 = 0;
        if (S.c0 >= n) S.c0 = n - 1;
        S.passes = 1;
    }
    __syncthreads();
    return true;
}

// ---- k-means++ (sklearn _kmeans_plusplus, n_local_trials = 2)
// Reads S.c0 and the caller's two draws; writes S.c1, the two centres S.cen (cenp, csnp zeroed)
// and passes.
template <class T>
SSF_DEV bool mask_kmeanspp(MaskCtx<T>& C, const MaskLds& L, const double* __restrict__ draws) {
    MaskShared& S = L.S;
    const int tid = threadIdx.x;
    const T* P = C.P;
    const T* Fl = C.Fl;
    const double (&mean)[6] = C.mean;
    const int64_t n = C.n, r0 = C.X.r0, r1 = C.X.r1;
    const int f = C.f;
    double c0[6], cn0 = 0.0;
    {
        double x[6];
        load_x(P, Fl, S.c0, x);
        for (int d = 0; d < 6; ++d) { c0[d] = x[d] - mean[d]; cn0 += c0[d] * c0[d]; }
    }
    // distances to the first centre; each wave owns a contiguous segment so the
    // in-order cumulative sum needs only one block-level exchange of wave totals
    const int nw = blockDim.x >> 6, w = tid >> 6, lane = lane_id();
    const int64_t nloc = r1 - r0;
    const int64_t seg = (((nloc + nw - 1) / nw) + 63) / 64 * 64;
    const int64_t ws = r0 + (int64_t)w * seg, we = ws + seg < r1 ? ws + seg : r1;
    // D(i) = squared distance to the first centre; recomputed (same expression, same bits)
    // wherever it is needed instead of being stored
    auto dist0x = [&](const double* x) {
        double dt = 0.0, xs = 0.0;
#pragma unroll
        for (int d = 0; d < 6; ++d) { const double v = x[d] - mean[d]; dt += c0[d] * v; xs += v * v; }
        const double v = (-2.0 * dt + cn0) + xs;
        return v > 0.0 ? v : 0.0;
    };
    auto dist0 = [&](int64_t i) {
        double x[6];
        load_x(P, Fl, i, x);
        return dist0x(x);
    };
    // the wave's segment streamed with the next kKppDeep blocks' points in flight (raw floats,
    // loads clamped and unconditional): each block was one dependent load latency before.
    // Diag stamps, B = 256: k-means++ 0.75 -> 0.56 M cycles per frame at depth 2; depth 4
    // 0.58 (tools/gpu/r3y.sh, r3z.sh)
    constexpr int kKppDeep = SSF_KPP_DEEP;
    const int64_t wlast = we > ws ? we - 1 : ws;
    // per 64-point block: the in-block inclusive scan's total (lane 63) goes to LDS, so the
    // draw search below only re-scans the one block that holds the draw
    const int64_t spw = seg / 64;                            // blocks per wave segment
    const bool use_blocks = spw * nw <= kKppBlocks;          // uniform
    double wsum = 0.0;
    T kb[kKppDeep][6];
    if (ws < we) {
#pragma unroll
        for (int k = 0; k < kKppDeep; ++k) load_raw_stream(P, Fl, min(ws + 64 * k + lane, wlast), kb[k]);
    }
    for (int64_t b0 = ws; b0 < we; b0 += 64 * kKppDeep)
#pragma unroll
    for (int k = 0; k < kKppDeep; ++k) {
        const int64_t b = b0 + 64 * k;
        if (b >= we) break;                                  // uniform
        const int64_t i = b + lane;
        double x[6];
#pragma unroll
        for (int d = 0; d < 6; ++d) x[d] = (double)kb[k][d];
        load_raw_stream(P, Fl, min(i + 64 * kKppDeep, wlast), kb[k]);
        const double d = i < we ? dist0x(x) : 0.0;
        wsum += d;
        if (use_blocks) {
            double v = d;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double y = __shfl_up(v, o, 64);
                if (lane >= o) v += y;
            }
            if (lane == 63) L.bsum[w * spw + (b - ws) / 64] = v;
        }
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
    if (tid == 0) S.passes += 1;
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
            double v = i < we ? dist0(i) : 0.0;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double y = __shfl_up(v, o, 64);
                if (lane >= o) v += y;
            }
            const double incl = (j ? cb2 : cb1) + v;
            const uint64_t mm = __ballot(i < we && incl >= (j ? t2 : t1));
            if (mm && lane == 0) atomicMin(&L.cand[j], (unsigned long long)(b + __ffsll((unsigned long long)mm) - 1));
        }
        f1 = f2 = true;                                      // skip the sequential scan
    }
    for (int64_t b = ws; b < we && !(f1 && f2); b += 64) {
        const int64_t i = b + lane;
        double v = i < we ? dist0(i) : 0.0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double y = __shfl_up(v, o, 64);
            if (lane >= o) v += y;
        }
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
    double cp[2] = {0.0, 0.0};
    if (ws < we) {
#pragma unroll
        for (int k = 0; k < kKppDeep; ++k) load_raw_stream(P, Fl, min(ws + 64 * k + lane, wlast), kb[k]);
    }
    for (int64_t b0 = ws; b0 < we; b0 += 64 * kKppDeep)
#pragma unroll
    for (int k = 0; k < kKppDeep; ++k) {
        const int64_t b = b0 + 64 * k;
        if (b >= we) break;                                  // uniform
        const int64_t i = b + lane;
        double x[6];
#pragma unroll
        for (int d = 0; d < 6; ++d) x[d] = (double)kb[k][d];
        load_raw_stream(P, Fl, min(i + 64 * kKppDeep, wlast), kb[k]);
        if (i < we) {
            double xs = 0.0, dt0 = 0.0, dt1 = 0.0, dtc = 0.0;
#pragma unroll
            for (int d = 0; d < 6; ++d) {
                const double v = x[d] - mean[d];
                dtc += c0[d] * v; xs += v * v; dt0 += cc[0][d] * v; dt1 += cc[1][d] * v;
            }
            double di = (-2.0 * dtc + cn0) + xs;             // = dist0(i), bit for bit
            di = di > 0.0 ? di : 0.0;
            double v0 = (-2.0 * dt0 + ccn[0]) + xs, v1 = (-2.0 * dt1 + ccn[1]) + xs;
            v0 = v0 > 0.0 ? v0 : 0.0; v1 = v1 > 0.0 ? v1 : 0.0;
            cp[0] += v0 < di ? v0 : di;
            cp[1] += v1 < di ? v1 : di;
        }
    }
    block_sum<2>(cp, L.red);
    if (!exchange<2>(C.X, cp, L.xtmp, &L.okflag)) return false;
    if (tid == 0) {
        const int best = cp[1] < cp[0] ? 1 : 0;
        S.c1 = cand[best];
        for (int d = 0; d < 6; ++d) { S.cen[d] = c0[d]; S.cen[6 + d] = cc[best][d]; }
        for (int d = 0; d < 12; ++d) S.cenp[d] = 0.0;
        S.csnp[0] = S.csnp[1] = 0.0;
        S.passes += 2;
    }
    __syncthreads();
    return true;
}

}  // namespace ssf
