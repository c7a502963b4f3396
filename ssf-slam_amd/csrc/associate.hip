// associate.hip -- the association of frameRegistration (src/lidarOdometry_onlyPC.cpp:147-252)
// on gfx950, batched over independent frame pairs.
//
// Per CURRENT plane point: transformToLast in double (:74-82) -> exact 1-NN in the last plane
// cloud (:168, unbounded) -> correspondence record {po, pa, n, valid} carrying the last frame's
// plane (plane_table.hip) for the solve (solve.hip).  launch_associate launches what
// register_plan chose:
//
//   k_associate_strips    last frames of up to kSortMax points: the strip image staged in LDS,
//                         1-NN by radius doubling over strip rings.  <kSoa, 0>: one query per
//                         lane (big launches; with one work-group per pair it writes the
//                         records compacted for the solve); <kSoa, kAssocCoopG>: one query per
//                         lane group (launches of at most kAssocCoopPairs pairs).  A last frame
//                         above the staging capacity walks the x-sorted copy in global memory.
//   k_associate           larger last frames (or no sorted copy): brute force.
#include "reg_strips.hpp"
#include "ssf_internal.hpp"

#include <algorithm>

namespace ssf {

__global__ __launch_bounds__(256) void k_associate(const float4* __restrict__ last,
                                                   const int64_t* __restrict__ last_off,
                                                   const int32_t* __restrict__ last_count,
                                                   const float* __restrict__ last_normal,
                                                   const uint8_t* __restrict__ last_valid,
                                                   const float4* __restrict__ curr,
                                                   const int64_t* __restrict__ curr_off,
                                                   const int32_t* __restrict__ curr_count,
                                                   const double* __restrict__ pose_rel,
                                                   CorrRec* __restrict__ corr,
                                                   int32_t* __restrict__ nn_out) {
    __shared__ float4 tile[kKnnTile];
    const int p = blockIdx.y;
    const int mc = curr_count[p], ml = last_count[p];
    if ((int)(blockIdx.x * blockDim.x) >= mc || ml <= 10) return;  // uniform (:158)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < mc;
    const float4* L = last + last_off[p];
    const int64_t co = curr_off[p];
    const double q[4] = {pose_rel[7 * p], pose_rel[7 * p + 1], pose_rel[7 * p + 2], pose_rel[7 * p + 3]};
    const double t[3] = {pose_rel[7 * p + 4], pose_rel[7 * p + 5], pose_rel[7 * p + 6]};
    float4 pc = make_float4(0.f, 0.f, 0.f, 0.f), qs = pc;
    if (active) {
        pc = curr[co + i];
        const double v[3] = {(double)pc.x, (double)pc.y, (double)pc.z};
        double r[3];
        quat_rotate(q, v, r);                                           // :74-82
        qs.x = (float)(r[0] + t[0]); qs.y = (float)(r[1] + t[1]); qs.z = (float)(r[2] + t[2]);
    }
    float best = __builtin_inff();
    int bi = -1;
    for (int t0 = 0; t0 < ml; t0 += kKnnTile) {
        const int nt = min(kKnnTile, ml - t0);
        for (int k = threadIdx.x; k < nt; k += blockDim.x) tile[k] = L[t0 + k];
        __syncthreads();
        if (active) {
            for (int k = 0; k < nt; ++k) {
                const float d = l2_simple(qs, tile[k]);
                if (d < best) { best = d; bi = t0 + k; }
            }
        }
        __syncthreads();
    }
    if (!active) return;
    const int64_t lo = last_off[p];
    CorrRec rec;
    const bool ok = bi >= 0 && last_valid[lo + bi];
    const float4 pa = L[bi >= 0 ? bi : 0];
    rec.po[0] = pc.x; rec.po[1] = pc.y; rec.po[2] = pc.z; rec.valid = ok ? 1.0f : 0.0f;
    rec.pa[0] = pa.x; rec.pa[1] = pa.y; rec.pa[2] = pa.z; rec.pad0 = 0.f;
    const float* nr = last_normal + 3 * (lo + (bi >= 0 ? bi : 0));
    rec.n[0] = nr[0]; rec.n[1] = nr[1]; rec.n[2] = nr[2]; rec.pad1 = 0.f;
    corr[co + i] = rec;
    if (nn_out) nn_out[co + i] = bi;
}

// Candidates are kept as a sorted rank bc; the original index (the tie-break key) is read only
// on an exact distance tie, and once at the end.
template <class V>
SSF_DEV bool assoc_better(const V& v, int c, float d, float best, int bc) {
    return d < best || (d == best && (bc < 0 || v.id(c) < v.id(bc)));
}

template <class V>
SSF_DEV void assoc_walk(const V& v, int ml, const float4& qs, float lim, float& best, int& bc) {
    int lo_i = 0, hi_i = ml;                                            // first x >= qs.x
    while (lo_i < hi_i) {
        const int mid = (lo_i + hi_i) >> 1;
        if (v.pt(mid).x < qs.x) lo_i = mid + 1; else hi_i = mid;
    }
    int c = lo_i;
    for (; c < ml; ++c) {
        const float4 pl = v.pt(c);
        const float dx = qs.x - pl.x;
        const float dx2 = dx * dx;
        if (dx2 > best || dx2 >= lim) break;
        const float d = l2_simple(qs, pl);
        if (assoc_better(v, c, d, best, bc)) { best = d; bc = c; }
    }
    int c2 = lo_i - 1;
    for (; c2 >= 0; --c2) {
        const float4 pl = v.pt(c2);
        const float dx = qs.x - pl.x;
        const float dx2 = dx * dx;
        if (dx2 > best || dx2 >= lim) break;
        const float d = l2_simple(qs, pl);
        if (assoc_better(v, c2, d, best, bc)) { best = d; bc = c2; }
    }
}

SSF_DEV void assoc_finish(const float4* __restrict__ L, int64_t lo, const float* __restrict__ last_normal,
                          const uint8_t* __restrict__ last_valid, const float4& pc, int bi,
                          CorrRec* __restrict__ corr, int32_t* __restrict__ nn_out, int64_t ci) {
    CorrRec rec;
    const bool ok = last_valid[lo + bi] != 0;
    const float4 pa = L[bi];
    rec.po[0] = pc.x; rec.po[1] = pc.y; rec.po[2] = pc.z; rec.valid = ok ? 1.0f : 0.0f;
    rec.pa[0] = pa.x; rec.pa[1] = pa.y; rec.pa[2] = pa.z; rec.pad0 = 0.f;
    const float* nr = last_normal + 3 * (lo + bi);
    rec.n[0] = nr[0]; rec.n[1] = nr[1]; rec.n[2] = nr[2]; rec.pad1 = 0.f;
    corr[ci] = rec;
    if (nn_out) nn_out[ci] = bi;
}

// ------------------------------------------------------------------------------------------
// Association over y-strips.  An x band around a query crosses every LiDAR ring: the 1-m walk
// visits ~60 candidates per query (the ~54 points inside |dx| < the final NN distance are
// unavoidable in x order), and the slowest lane of a wave ~217.  One work-group per pair stages
// the last frame (x-sorted) into LDS partitioned into strips of width W >= 1 m in y, x order
// kept inside each strip (stable partition: per-wave match masks on the strip id + per-wave
// strip counts, chunk by chunk in x order).  A query searches its own strip (binary search in
// x, outward walk while dx^2 + dymin^2 <= best), then the strips above and below, ring by
// ring, while a lower bound of their |dy| can still beat the best: ~8 candidates per query,
// every query exact (no 1-m band, no exhaustive phase).  Lower bounds: inside a searched strip,
// dymin from the strip's actual y extent (fl(qy - yhi) <= fl(qy - py) by monotone rounding, so
// fl(fl(dx^2) + fl(dymin^2)) <= the float distance); for the ring stop, the nominal strip edge
// minus strip_slack: 1 mm or, on extents of kilometres, 16 eps (|y0| + |y1| + |qy|) (float strip
// assignment; derived in reg_strips.hpp).  Candidates compare as (distance, original index).
// kSoa: the strip-major points as x | y | z float arrays and a u16 original index (configs[4]
// frames); otherwise float4 with the index in .w.  A last frame above the launch's staging
// capacity walks the x-sorted copy in global memory, unbounded (exact, slow, not expected).
// kCoopG > 0 (launches of few pairs: a node's one pair, configs[2]'s chained pairs): one query
// per group of kCoopG lanes instead of one per lane -- the query's strips of each search level
// spread over the group's lanes (one strip per lane), so no lane walks ring after ring alone,
// and (kStripThreads / kCoopG) queries per work-group over ceil(m / that) work-groups per pair
// (each stages the last frame).  The lane mode's nested divergent loops (levels, rings, walks)
// leave a wave at the pace of its slowest lane: SQ counters in the chain, r5w: ~138 LDS
// instructions per wave over ~51 k wave-cycles, 56 % of them waiting.
#ifndef SSF_ASSOC_COOP_G
#define SSF_ASSOC_COOP_G 16
#endif
constexpr int kAssocCoopG = SSF_ASSOC_COOP_G;
constexpr int kAssocCoopPairs = 16;             // launches of at most this many pairs take the group mode
template <bool kSoa, int kCoopG = 0>
__global__ __launch_bounds__(kStripThreads) void k_associate_strips(
    const float4* __restrict__ last, const int64_t* __restrict__ last_off,
    const int32_t* __restrict__ last_count, const float* __restrict__ last_normal,
    const uint8_t* __restrict__ last_valid, const float4* __restrict__ last_sorted,
    const int32_t* __restrict__ last_sidx, const float4* __restrict__ curr,
    const int64_t* __restrict__ curr_off, const int32_t* __restrict__ curr_count,
    const double* __restrict__ pose_rel, CorrRec* __restrict__ corr, int32_t* __restrict__ nn_out,
    int lds_cap, const float4* __restrict__ strip_xyzi, const int32_t* __restrict__ strip_head,
    int32_t* __restrict__ nnv, int32_t* __restrict__ ncompact) {
    extern __shared__ float4 SL[];                  // [ml] strip-major, x-sorted in each strip
    __shared__ StripLds T;
    // Compacted records (round 6): with one work-group per pair in the lane mode, the valid
    // correspondences are written in query order at their ranks, [0, ncompact[p]) of the pair's
    // records (a pair whose records are not compacted gets -1): k_solve then streams them into its
    // LDS with no ballot pass and evaluates them on the way in.  Each query's (1-NN index, valid)
    // goes to nnv first; the ranks need every query's validity.
    const bool compact = kCoopG == 0 && ncompact && gridDim.y == 1;   // uniform
    __shared__ int cwave[kStripWaves];
    // gridDim.y work-groups per pair (few pairs in a launch): each stages the whole last frame
    // and answers every gridDim.y-th block of kStripThreads queries
    const int p = blockIdx.x, tid = threadIdx.x;
    const int q0 = tid + (int)blockIdx.y * kStripThreads, qstep = kStripThreads * (int)gridDim.y;
    const int mc = curr_count[p], ml = last_count[p];
    if (mc <= 0 || ml <= 10) {                                          // uniform (:158)
        if (compact && tid == 0) ncompact[p] = 0;
        return;
    }
    constexpr int kQpw = kCoopG > 0 ? kStripThreads / kCoopG : kStripThreads;   // queries per work-group
    if (kCoopG > 0 && (int)blockIdx.y * kQpw >= mc) return;             // uniform: no query here
    const int64_t lo = last_off[p], co = curr_off[p];
    const float4* SP = last_sorted + lo;
    const int32_t* SI = last_sidx + lo;
    const double q[4] = {pose_rel[7 * p], pose_rel[7 * p + 1], pose_rel[7 * p + 2], pose_rel[7 * p + 3]};
    const double t[3] = {pose_rel[7 * p + 4], pose_rel[7 * p + 5], pose_rel[7 * p + 6]};
    const float4* L = last + lo;
#ifdef SSF_STRIPS_STAMPS
    // diagnostic build only: per work-group s_memrealtime (100 MHz) and s_memtime (core clock)
    // at entry, after the staging and after the queries, into nn_out[co + 8 y ..] at the end
    const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime(), mt0 = __builtin_amdgcn_s_memtime();
    unsigned long long rt1 = rt0, mt1 = mt0;
#endif
    if (ml > lds_cap) {                                                 // uniform
        if (compact && tid == 0) ncompact[p] = -1;                      // records in query order
        const PtsF4 g{SP, SI};
        for (int i = q0; i < mc; i += qstep) {
            const float4 pc = curr[co + i];
            const float4 qs = assoc_query_point(pc, q, t);
            float best = __builtin_inff();
            int bc = -1;
            assoc_walk(g, ml, qs, __builtin_inff(), best, bc);
            assoc_finish(L, lo, last_normal, last_valid, pc, g.id(max(bc, 0)), corr, nn_out, co + i);
        }
        return;
    }
    float* SX = reinterpret_cast<float*>(SL);
    uint16_t* SI16 = reinterpret_cast<uint16_t*>(SX + 3 * ml);
    // the plane table's image of this last frame when the caller kept it (a copy: ~4 us of the
    // ~40 us build), otherwise the build
    const StripGeo geo = (!kSoa && strip_xyzi && strip_image_frame(ml) && strip_image_valid(strip_head + lo))
        ? strip_image_load(strip_xyzi + lo, strip_head + lo, ml, SL, T)
        : strips_build<kSoa, kStripPerMax>(
              [&](int, int r) { float4 pt = SP[r]; pt.w = __int_as_float(SI[r]); return pt; }, ml, T, SL, SX, SI16);
    const float y0 = geo.y0, W = geo.W;
    const int ns = geo.ns;
    const float span = geo.span();
    auto strip_of = [&](float y) { return geo.strip_of(y); };
    const StripView<kSoa> v{SL, SX, SI16, ml};
#ifdef SSF_STRIPS_STAMPS
    rt1 = __builtin_amdgcn_s_memrealtime(); mt1 = __builtin_amdgcn_s_memtime();
#else
    if (kCoopG == 0 && q0 >= mc && !compact) return;                    // (after the barriers of the build)
#endif
#ifdef SSF_ASSOC_COUNT
    int vis = 0;
#endif
    // one strip: points with dx^2 + dymin^2 <= min(best, lim) (lim = R^2 of the search radius)
    auto search = [&](int sidx, float lim, const float4& qs, float& best, int& bc) __attribute__((always_inline)) {
        const int a = T.start[sidx], b = T.start[sidx + 1];
        if (a >= b) return;
        const float yl = T.ylo[sidx], yh = T.yhi[sidx];
        const float dyl = qs.y < yl ? yl - qs.y : (qs.y > yh ? qs.y - yh : 0.0f);
        const float dy2 = dyl * dyl;
        if (dy2 > fminf(best, lim)) return;
#ifdef SSF_ASSOC_COUNT
        vis += 1 << 16;                                                  // strip searches (high half)
#endif
        int l = a, h = b;                                                // first x >= qs.x
        while (l < h) {
            const int mid = (l + h) >> 1;
            if (v.x(mid) < qs.x) l = mid + 1; else h = mid;
        }
        // the next record is read while the current one is processed (clamped into the strip)
        if (l < b) {
            float4 pn = v.pt(l);
            for (int c = l; c < b; ++c) {
                const float4 pl = pn;
                pn = v.pt(min(c + 1, b - 1));
                const float dx = qs.x - pl.x;
                if (dx * dx + dy2 > fminf(best, lim)) break;
                const float d = l2_simple(qs, pl);
                if (assoc_better(v, c, d, best, bc)) { best = d; bc = c; }
#ifdef SSF_ASSOC_COUNT
                ++vis;
#endif
            }
        }
        if (l > a) {
            float4 pn = v.pt(l - 1);
            for (int c = l - 1; c >= a; --c) {
                const float4 pl = pn;
                pn = v.pt(max(c - 1, a));
                const float dx = qs.x - pl.x;
                if (dx * dx + dy2 > fminf(best, lim)) break;
                const float d = l2_simple(qs, pl);
                if (assoc_better(v, c, d, best, bc)) { best = d; bc = c; }
#ifdef SSF_ASSOC_COUNT
                ++vis;
#endif
            }
        }
    };
    if (kCoopG > 0) {
        // one query per kCoopG-lane group (groups are aligned lane ranges: the reductions stay
        // inside one), the same levels and bounds as the lane mode below
        const int gl = tid % kCoopG;
        for (int i = (int)blockIdx.y * kQpw + tid / kCoopG; i < mc; i += (int)gridDim.y * kQpw) {   // uniform per group
            const float4 pc = curr[co + i];
            const float4 qs = assoc_query_point(pc, q, t);
            float best = __builtin_inff();
            int bc = -1;
            unsigned long long key = ~0ull;
            for (float R = 2.0f;; R *= 2.0f) {
                const bool unbounded = R > 4096.0f;
                const float lim = unbounded ? __builtin_inff() : R * R;
                // the whole W added here, not the 1 mm, carries the float error of the strip
                // assignment at large extents (strip_of is monotone: a point within R of qs.y in
                // y is in [sa, sb] already without either)
                const int sa = unbounded ? 0 : strip_of(qs.y - R - W - 1e-3f);
                const int sb = unbounded ? ns - 1 : strip_of(qs.y + R + W + 1e-3f);
                for (int sidx = sa + gl; sidx <= sb; sidx += kCoopG) search(sidx, lim, qs, best, bc);
                unsigned long long k = bc >= 0
                    ? ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)v.id(bc) : ~0ull;
#pragma unroll
                for (int o = kCoopG / 2; o >= 1; o >>= 1) {
                    const unsigned long long x = __shfl_xor(k, o, kWave);
                    k = x < k ? x : k;
                }
                key = k < key ? k : key;
                const float wb = key == ~0ull ? __builtin_inff() : __uint_as_float((unsigned)(key >> 32));
                if (wb <= lim || unbounded) break;
                best = wb; bc = -1;
            }
            if (gl == 0) {
                // no candidate at all (a NaN query, e.g. after a NaN warm start): the lane mode's
                // fallback, sorted rank 0, instead of index -1
                assoc_finish(L, lo, last_normal, last_valid, pc, key == ~0ull ? v.id(0) : (int)(key & 0xffffffffu),
                             corr, nn_out, co + i);
#ifdef SSF_ASSOC_COUNT
                if (nn_out) nn_out[co + i] = vis;
#endif
            }
        }
    }
    for (int i = q0; i < (kCoopG > 0 ? 0 : mc); i += qstep) {
        const float4 pc = curr[co + i];
        const float4 qs = assoc_query_point(pc, q, t);
        float best = __builtin_inff();
        int bc = -1;
#ifdef SSF_ASSOC_COUNT
        vis = 0;
#endif
        // Radius doubling (R = 2, 4, 8, ... m, then unbounded): a level visits, strip ring by
        // strip ring from the query's, every point with dx^2 + dymin^2 <= min(best, R^2).  Once
        // best <= R^2 every point as close as best has been seen (its lower bound is <= its
        // distance <= best <= R^2), so the 1-NN is exact; a query in an empty region (a masked
        // hole, BASELINE configs[2]) therefore walks the points within ~2x its 1-NN distance,
        // not every point within the distance of the first point its own strip happens to hold.
        const int s0 = strip_of(qs.y);
        const float slack = strip_slack(span, qs.y);                     // reg_strips.hpp
        for (float R = 2.0f;; R *= 2.0f) {
            const bool unbounded = R > 4096.0f;                          // uniform per lane
            const float lim = unbounded ? __builtin_inff() : R * R;
            search(s0, lim, qs, best, bc);
            bool up = true, dn = true;
            for (int rr = 1; up || dn; ++rr) {
                const float bnd = fminf(best, lim);
                if (up) {
                    const int su = s0 + rr;
                    // every point of strips >= su has y >= y0 + su W (less float slack)
                    const float gap = (y0 + (float)su * W) - qs.y - slack;
                    if (su >= ns || (gap > 0.0f && gap * gap > bnd)) up = false;
                    else search(su, lim, qs, best, bc);
                }
                if (dn) {
                    const int sd = s0 - rr;
                    const float gap = qs.y - (y0 + (float)(sd + 1) * W) - slack;
                    if (sd < 0 || (gap > 0.0f && gap * gap > bnd)) dn = false;
                    else search(sd, lim, qs, best, bc);
                }
            }
            if (best <= lim || unbounded) break;
        }
        if (compact) {
            // the 1-NN's LDS position (its point and index are read back from the strips)
            const int bp = max(bc, 0), bi = v.id(bp);
            nnv[co + i] = last_valid[lo + bi] != 0 ? bp : -1 - bp;      // read back by this thread
            if (nn_out) nn_out[co + i] = bi;
        } else {
            assoc_finish(L, lo, last_normal, last_valid, pc, v.id(max(bc, 0)), corr, nn_out, co + i);
        }
#ifdef SSF_ASSOC_COUNT
        if (nn_out) nn_out[co + i] = vis;
#endif
    }
    if (compact) {
        // query trip k (queries k T + tid, T = kStripThreads: the lane loop's own, so every thread
        // reads back its own nnv entries): ballot + wave counts give the ranks in query order
        const int lane = tid & 63, w = tid >> 6;
        int base = 0;                                                   // uniform
        for (int i0 = 0; i0 < mc; i0 += kStripThreads) {
            const int i = i0 + tid;
            const int e = i < mc ? nnv[co + i] : -1;
            const bool val = e >= 0;
            const uint64_t m = __ballot(val);
            if (lane == 0) cwave[w] = __popcll(m);
            __syncthreads();
            int before = base, tot = 0;
#pragma unroll
            for (int j = 0; j < kStripWaves; ++j) { const int x = cwave[j]; if (j < w) before += x; tot += x; }
            if (val) {
                CorrRec rec;
                const float4 pc = curr[co + i], pa = v.pt(e);                 // pa: L[bi]'s floats
                const float* nr = last_normal + 3 * (lo + v.id(e));
                rec.po[0] = pc.x; rec.po[1] = pc.y; rec.po[2] = pc.z; rec.valid = 1.0f;
                rec.pa[0] = pa.x; rec.pa[1] = pa.y; rec.pa[2] = pa.z; rec.pad0 = 0.f;
                rec.n[0] = nr[0]; rec.n[1] = nr[1]; rec.n[2] = nr[2]; rec.pad1 = 0.f;
                corr[co + before + __popcll(m & lanemask_lt())] = rec;
            }
            base += tot;
            __syncthreads();                                            // cwave is rewritten next trip
        }
        if (tid == 0) ncompact[p] = base;
    }
#ifdef SSF_STRIPS_STAMPS
    __syncthreads();
    if (tid == 0 && nn_out) {
        const unsigned long long rt2 = __builtin_amdgcn_s_memrealtime(), mt2 = __builtin_amdgcn_s_memtime();
        int32_t* o = nn_out + co + kQpw * blockIdx.y;                // this work-group's own query slots
        o[0] = (int32_t)(rt1 - rt0); o[1] = (int32_t)(rt2 - rt0);
        o[2] = (int32_t)(rt2 - rt0); o[3] = 0;
        (void)mt1; (void)mt2;
        o[4] = (int32_t)(rt0 & 0x7fffffff); o[5] = __smid();
        o[6] = (int32_t)(strip_xyzi && strip_image_frame(ml) && strip_image_valid(strip_head + lo));
        o[7] = ml;
    }
#endif
}

// The choice launch_register makes for a launch's association on the kSortMax strip path (host
// only, no HIP call; ssf_register_plan exports it so that tests can prove which path a launch
// took).  Few pairs (a node's one pair, configs[2]'s chained pairs) take the group mode: up to 8
// work-groups per pair, each staging the last frame and taking a share of the queries, so the
// launch spreads over ~256 CUs instead of n_pairs (every work-group stages the whole last frame,
// so the split is capped at ~4 launch-filling waves of work-groups; the query loop strides over
// gridDim.y).  Big launches: the lane mode, split over
// min(8, 256 / n_pairs, ceil(max_m / kStripThreads)) work-groups per pair; with ONE work-group
// per pair and planes only, the association hands the solve compacted records.
RegisterPlan register_plan(int n_pairs, int64_t max_m, bool with_edges) {
    RegisterPlan r{};
    if (n_pairs <= 0 || max_m <= 0 || max_m > kSortMax) return r;
    r.strips = true;
    r.soa = max_m > kAssocStripF4Max;
    r.lds_cap = (int)std::min<int64_t>(max_m, r.soa ? kAssocStripSoaMax : kAssocStripF4Max);
    r.coop = n_pairs <= kAssocCoopPairs;
    constexpr int kQpwCoop = kStripThreads / kAssocCoopG;
    r.qsplit = r.coop ? (int)std::min<int64_t>((max_m + kQpwCoop - 1) / kQpwCoop,
                                               std::max(8, 1024 / n_pairs))
                      : (int)std::max<int64_t>(1, std::min<int64_t>({8, 256 / n_pairs,
                                               (max_m + kStripThreads - 1) / kStripThreads}));
    r.compacted = !r.coop && r.qsplit == 1 && !with_edges;
    return r;
}

// The association launch of launch_register: the path `plan` names (register_plan, its strips /
// compacted flags already cleared by the caller when the sorted copy / the nnv and ncompact
// scratch are missing).
void launch_associate(hipStream_t s, int n_pairs, const RegisterPlan& plan, const RegisterArgs& a,
                      const double* pin) {
    const RegFrames &last = a.last, &curr = a.curr;
    const RegTable& t = a.table;
    if (plan.strips) {
        const bool soa = plan.soa, coop = plan.coop;
        const int cap = plan.lds_cap, qsplit = plan.qsplit;
        const size_t lds = soa ? (size_t)cap * 14 + 16 : (size_t)cap * sizeof(float4);
        int32_t* ncp = plan.compacted ? a.scratch.ncompact : nullptr;
        kmark(s, coop ? "k_associate_strips_coop" : soa ? "k_associate_strips_soa" : "k_associate_strips");
        hipLaunchKernelGGL(coop ? (soa ? k_associate_strips<true, kAssocCoopG> : k_associate_strips<false, kAssocCoopG>)
                                : (soa ? k_associate_strips<true> : k_associate_strips<false>),
                           dim3(n_pairs, qsplit), dim3(kStripThreads), lds, s, last.xyzi, last.off, last.count,
                           t.normal, t.valid, t.sorted, t.sidx, curr.xyzi, curr.off,
                           curr.count, pin, a.scratch.corr, a.out.nn, cap,
                           t.strip_head ? t.strip_xyzi : nullptr, t.strip_head,
                           ncp ? a.scratch.nnv : nullptr, ncp);
    } else {
        const int bx = (int)((a.max_m + 255) / 256);
        kmark(s, "k_associate");
        hipLaunchKernelGGL(k_associate, dim3(bx, n_pairs), dim3(256), 0, s, last.xyzi, last.off,
                           last.count, t.normal, t.valid, curr.xyzi, curr.off, curr.count,
                           pin, a.scratch.corr, a.out.nn);
    }
}

}  // namespace ssf
