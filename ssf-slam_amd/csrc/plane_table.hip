// plane_table.hip -- the plane table of lidarOdometry_onlyPC::frameRegistration
// (src/lidarOdometry_onlyPC.cpp:147-252) on gfx950, batched over independent frames.
//
// Per LAST-frame plane point a: exact 30-NN (FLANN L2_Simple float distances, ties to the lower
// index), ring-diverse 5-point pick (:180-205), gate d2[n] < 1 (:207), 5x3 column-pivoted
// Householder least squares (:208-220), coplanarity gate (:222-232).  It depends only on (last
// frame, a), so it is computed once per frame instead of twice per correspondence.
// launch_plane_table picks the kernel:
//
//   k_plane_table_sorted  frames of up to kSortMax plane points: one work-group per frame sorts
//                         it by x (rocPRIM radix sort), rebuilds it as y-strips in LDS and
//                         answers every query from a bounded walk over three strips; writes the
//                         sorted copy and the strip image the association reuses.
//   k_plane_table         larger frames: brute force over the frame streamed through LDS tiles.
//   k_strip_invalidate    marks the strip images stale after a k_plane_table launch.
#include "reg_strips.hpp"
#include "ssf_internal.hpp"

#include <algorithm>

#include <rocprim/block/block_radix_sort.hpp>

namespace ssf {

__global__ __launch_bounds__(256) void k_plane_table(const float4* __restrict__ plane,
                                                     const int64_t* __restrict__ frame_off,
                                                     const int32_t* __restrict__ count,
                                                     float plane_max, float* __restrict__ normal,
                                                     uint8_t* __restrict__ valid) {
    __shared__ float4 tile[kKnnTile];
    const int f = blockIdx.y;
    const int m = count[f];
    if ((int)(blockIdx.x * blockDim.x) >= m) return;  // uniform
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = a < m;
    const float4* P = plane + frame_off[f];
    const float4 q = active ? P[a] : make_float4(0.f, 0.f, 0.f, 0.f);
    double kk[kK];
#pragma unroll
    for (int k = 0; k < kK; ++k) kk[k] = knn_key(__builtin_inff(), 0x7fffffff);
    for (int t0 = 0; t0 < m; t0 += kKnnTile) {
        const int nt = min(kKnnTile, m - t0);
        for (int k = threadIdx.x; k < nt; k += blockDim.x) tile[k] = P[t0 + k];
        __syncthreads();
        if (active) {
            for (int k = 0; k < nt; ++k) {
                const double key = knn_key(l2_simple(q, tile[k]), t0 + k);
                if (key < kk[kK - 1]) key_insert<kK>(kk, key);
            }
        }
        __syncthreads();
    }
    if (!active) return;
    float nrm[3];
    uint8_t ok;
    plane_from_knn(P, kk, m, plane_max, nrm, ok);
    const int64_t o = frame_off[f] + a;
    normal[3 * o] = nrm[0]; normal[3 * o + 1] = nrm[1]; normal[3 * o + 2] = nrm[2];
    valid[o] = ok;
}

// ------------------------------------------------------------------------------------------
// x-sorted exact k-NN.  One work-group per frame bitonic-sorts the frame's plane points by
// (x, index) in LDS; every query then walks outward from its own position in x order and stops a
// direction once fl(dx*dx) exceeds its current K-th distance: since the float distance
// ((dx*dx + dy*dy) + dz*dz) >= fl(dx*dx) and fl(dx*dx) grows monotonically along the sorted
// order, no point beyond the stop can enter the list.  Lists are ordered by (distance, original
// index), so the result is exactly the brute-force (index-order) result.  Typical frames touch a
// few hundred candidates per query instead of all M.  The sorted points / permutation are
// written out and reused as the LAST frame of the next pair's association.
constexpr int kTableThreads = 1024;
#ifndef SSF_TABLE_MAX_SPLIT
#define SSF_TABLE_MAX_SPLIT 8                     // work-groups per frame at most (small batches)
#endif

// Diagnostic build only (-DSSF_TABLE_STAMPS): lane 0 writes s_memtime deltas after the sort,
// the bounded walks and the deferred walks into sorted_idx[m .. m+3] (frame padding, read by
// tools/diag_table_phases.py); the product library never executes it.
#ifdef SSF_TABLE_STAMPS
#define SSF_TSTAMP(k) do { __syncthreads(); if (threadIdx.x == 0) SI[m + (k)] = (int32_t)((__builtin_amdgcn_s_memtime() - tstamp0) >> 4); } while (0)
#else
#define SSF_TSTAMP(k) do { } while (0)
#endif

// Outward x-walk from sorted rank r.  bounded: the list is seeded with the sentinel distance 1,
// so only points with d2 < 1 enter it, and the walk stops once dx^2 >= 1 (only those points are
// needed to decide most queries, see bounded_decides).
template <class V>
SSF_DEV void knn_walk(const V& v, int m, int r, const float4& q, bool bounded, double (&kk)[kK]) {
    const float lim = bounded ? 1.0f : __builtin_inff();
#pragma unroll
    for (int k = 0; k < kK; ++k) kk[k] = knn_key(lim, 0x7fffffff);
    for (int c = r; c < m; ++c) {                         // rightwards (x non-decreasing)
        const float4 p = v.pt(c);
        const float dx = q.x - p.x;
        const float dx2 = dx * dx;
        if (dx2 > key_dist(kk[kK - 1]) || dx2 >= lim) break;
        const double key = knn_key(l2_simple(q, p), v.id(c));
        key_insert<kK>(kk, key);              // branch-free: a key >= kk[K-1] passes through
    }
    for (int c = r - 1; c >= 0; --c) {                    // leftwards
        const float4 p = v.pt(c);
        const float dx = q.x - p.x;
        const float dx2 = dx * dx;
        if (dx2 > key_dist(kk[kK - 1]) || dx2 >= lim) break;
        const double key = knn_key(l2_simple(q, p), v.id(c));
        key_insert<kK>(kk, key);              // branch-free: a key >= kk[K-1] passes through
    }
}

// Is the 1-m-bounded list (kd, ki) enough to reproduce :177-232 exactly?  Let K1 = #points with
// d2 < 1 (all of them are in the list: they have |dx| < 1).  The gate d2[n] < 1 (:207) holds iff
// n < K1.  K1 <= 5 -> n >= 5 fails;  K1 >= 30 -> the list is the exact 30-NN;  two qualifying
// different-row points among ranks 5..K1-1 -> n < K1 and only ranks < K1 are used.  Otherwise
// the answer depends on ranks beyond 1 m and the query takes the full walk.
// returns 0 undecided, 1 decided (the list is exact for every rank the pick uses), 2 decided
// invalid (K1 <= 5: the list may be short, the plane is rejected without reading it).
SSF_DEV int bounded_decides(const float4* __restrict__ P, int m, const double (&kk)[kK]) {
    if (m <= kK) return 0;
    int K1 = 0;
#pragma unroll
    for (int k = 0; k < kK; ++k) K1 += key_dist(kk[k]) < 1.0f;
    if (K1 <= 5) return 2;
    if (K1 >= kK) return 1;
    const int prow = row_of(P[key_index(kk[0])].w);
    int nq = 0;
#pragma unroll
    for (int k = 5; k < kK; ++k)
        if (k < K1) {
            const int row = row_of(P[key_index(kk[k])].w);
            nq += (row != prow && row >= 0 && row <= 63);
        }
    return nq >= 2 ? 1 : 0;
}

// A deferred query has 6 <= K1 < 30 keys inside 1 m.  bounded_decides defers it because fewer
// than two other-ring points (rings 0..63) lie among ranks 5..K1-1 -- or, in a frame of at most
// kK points, whatever it holds.  nq counts those points (the keys are in rank order, so every key
// inside 1 m comes before the first beyond it):
//   nq >= 2  the pick (lidarOdometry_onlyPC.cpp:180-198) stops at the second of them, inside
//            1 m; no point beyond 1 m can invalidate it and the plane uses only exact ranks;
//   nq < 2   the plane is valid only if NO point of ranks K1..29 lies on another ring: the pick
//            takes the first such point, n becomes its rank and dis2[n] >= 1 fails :207.  If none
//            is there, n is a rank inside 1 m and the plane uses only points inside 1 m.
// kk is exact for every key closer than lim.  Returns 1 when the list is complete or nq >= 2
// (table_finish decides), 2 when an other-ring point among the exact ranks >= K1 decides it
// invalid, 0 when the ranks beyond lim are still needed.
SSF_DEV int deferred_decides(const float4* __restrict__ P, const double (&kk)[kK], float lim) {
    if (key_dist(kk[kK - 1]) < lim) return 1;
    const int prow = row_of(P[key_index(kk[0])].w);
    int dec = 0, nq = 0;
#pragma unroll
    for (int k = 5; k < kK; ++k) {
        const float d = key_dist(kk[k]);
        if (d < lim) {
            const int row = row_of(P[key_index(kk[k])].w);
            const bool other = row != prow && row >= 0 && row <= 63;
            if (d < 1.0f) nq += other;
            else if (other && nq < 2) dec = 2;
        }
    }
    return nq >= 2 ? 1 : dec;
}

SSF_DEV void table_finish(const float4* __restrict__ P, int m, float plane_max, int64_t o,
                          const double (&kk)[kK], float* __restrict__ normal,
                          uint8_t* __restrict__ valid) {
    float nrm[3];
    uint8_t ok;
    plane_from_knn(P, kk, m, plane_max, nrm, ok);
    normal[3 * o] = nrm[0]; normal[3 * o + 1] = nrm[1]; normal[3 * o + 2] = nrm[2];
    valid[o] = ok;
}

// Queries in sorted order (adjacent lanes ~ adjacent x): 1-m-bounded walk for everyone; the
// undecided few go to an LDS queue and are re-walked in full afterwards, one per lane, so a
// handful of long walks no longer stalls whole waves.  queue == nullptr: walk in full at once.
template <class V>
SSF_DEV void table_walks(const float4* __restrict__ P, const V& v, int m, float plane_max,
                         int64_t base, float* __restrict__ normal, uint8_t* __restrict__ valid,
                         int* queue, int qcap, int* qlen, int32_t* stamp_out = nullptr,
                         unsigned long long stamp0 = 0) {
    for (int r = threadIdx.x; r < m; r += blockDim.x) {
        const float4 q = v.pt(r);
        double kk[kK];
        bool bounded = true;
        int dec;
        for (;;) {                                        // one walk call site: one live list
            knn_walk(v, m, r, q, bounded, kk);
            if (!bounded) { dec = 1; break; }
            dec = bounded_decides(P, m, kk);
            if (dec != 0) break;
            const int slot = queue ? atomicAdd(qlen, 1) : qcap;
            if (slot < qcap) { queue[slot] = r; break; }
            bounded = false;
        }
        if (dec == 2) {                                   // gate d2[n] < 1 fails for any n >= 5
            const int64_t o = base + v.id(r);
            normal[3 * o] = 0.f; normal[3 * o + 1] = 0.f; normal[3 * o + 2] = 0.f;
            valid[o] = 0;
        } else if (dec == 1) {
            table_finish(P, m, plane_max, base + v.id(r), kk, normal, valid);
        }
    }
    if (!queue) return;
    __syncthreads();
#ifdef SSF_TABLE_STAMPS
    if (threadIdx.x == 0 && stamp_out) *stamp_out = (int32_t)((__builtin_amdgcn_s_memtime() - stamp0) >> 4);
    if (threadIdx.x == 0 && stamp_out) stamp_out[1] = *qlen;
#endif
    const int nq = min(*qlen, qcap);
    for (int k = threadIdx.x; k < nq; k += blockDim.x) {
        const int r = queue[k];
        const float4 q = v.pt(r);
        double kk[kK];
        knn_walk(v, m, r, q, false, kk);
        table_finish(P, m, plane_max, base + v.id(r), kk, normal, valid);
    }
}

// The table's walks over the strips, queries in strip-major order (adjacent lanes: the same
// strip, adjacent x).  1-m bounded search for everyone; the undecided few are queued and
// searched in full afterwards (as table_walks).
#ifndef SSF_DEFER_RINGS
#define SSF_DEFER_RINGS 6
#endif
constexpr int kDeferRings = SSF_DEFER_RINGS;     // deferred queries: strips within this many metres
#ifndef SSF_DEFER_FIRST
#define SSF_DEFER_FIRST 2
#endif
constexpr int kDeferFirst = SSF_DEFER_FIRST;     // ... searched first within this many metres

SSF_DEV void table_deferred_walk(const float4* __restrict__ P, const float4* __restrict__ SP,
                                 const int32_t* __restrict__ SI, int m, int qi, const float4& q,
                                 double (&kk)[kK]) {
    int l = 0, h = m;                                  // x rank of (q.x, qi) in the sorted copy
    while (l < h) {
        const int mid = (l + h) >> 1;
        if (lex_less(SP[mid].x, SI[mid], q.x, qi)) l = mid + 1; else h = mid;
    }
    knn_walk(PtsF4{SP, SI}, m, l, q, false, kk);
}

// ---- the plane table's pick without the 30-key list (16-B strip layout) ---------------------
// The pick (lidarOdometry_onlyPC.cpp:180-207) reads, from the sorted 30-NN list: the ranks 0..4,
// prow = the row of rank 0, and in rank order from rank 5 the first two points on another ring
// (0..63); n = the rank of the last one found (5 if none) must satisfy d2[n] < 1.  With K1 = the
// number of points within 1 m (the query itself included):
//   K1 <= 5                      -> invalid (n >= 5 >= K1);
//   D1 < D2: the two smallest keys of other-ring points of rank >= 5 within 1 m;
//   K1 >= 30                     -> n = rank of the last of D1, D2 whose rank (= number of keys
//                                   below it) is < 30, else 5; always valid-gated (d2 < 1);
//   K1 < 30, D2 found            -> n = rank(D2) < K1, D1 and D2 replace ranks 3 and 4;
//   K1 < 30, D2 not found        -> the ranks K1..29 lie beyond 1 m: the plane is invalid iff
//                                   an other-ring point has rank < 30, i.e. iff E, the smallest
//                                   key of an other-ring point beyond 1 m, has fewer than
//                                   30 - K1 keys beyond 1 m below it; else valid with D1 (if any).
// The planes are computed from the same five points as plane_from_knn; each stage walks the
// strips with a few registers instead of inserting every candidate into a 30-key list.
constexpr uint32_t kRowCodeBad = 255u;
SSF_DEV uint32_t row_code(float fi) {
    const int r = row_of(fi);
    return (r >= 0 && r < (int)kRowCodeBad) ? (uint32_t)r : kRowCodeBad;
}
SSF_DEV int pt_row(const float4& p) { return (__float_as_int(p.w) >> 16) & 0xFF; }
SSF_DEV int pt_id(const float4& p) { return __float_as_int(p.w) & 0xFFFF; }
// The pick walks' keys carry the point's ring code too (round 6): low word = index << 8 | ring
// code.  Indices are unique, so the key order is still exactly (distance, index); a key that
// leaves the top-five list tells its ring by itself (pick_1m keeps two other-ring keys instead of
// six).  The sentinel knn_key(d, 0x7fffffff) decodes as ring 255 (never another ring in 0..63).
SSF_DEV double pick_key(float d, const float4& p) {
    const int w = __float_as_int(p.w);
    return __hiloint2double(__float_as_int(d), ((w & 0xFFFF) << 8) | ((w >> 16) & 0xFF));
}
SSF_DEV int pick_index(double k) { return (int)((uint32_t)__double2loint(k) >> 8); }
SSF_DEV int pick_row(double k) { return __double2loint(k) & 0xFF; }

// Visit the points of one strip with dx^2 + dy_lb^2 <= bound() (bound re-read at every step)
// and < lim, from q's x position (start: the query's own strip position, or -1 = binary search).
// start: in, the query's own strip position or a position found before; -1: binary search
// (the result is stored back, so later walks of the same strip skip the search).
template <class Bound, class Body>
SSF_DEV void strip_visit(const StripView<false>& v, const StripLds& T, int sidx, int& start, const float4& q,
                         float lim, Bound&& bound, Body&& body) {
    const int a = T.start[sidx], b = T.start[sidx + 1];
    if (a >= b) return;
    const float yl = T.ylo[sidx], yh = T.yhi[sidx];
    const float dyl = q.y < yl ? yl - q.y : (q.y > yh ? q.y - yh : 0.0f);
    const float dy2 = dyl * dyl;
    if (dy2 > bound() || dy2 >= lim) return;
    int l = start;
    if (l < 0) {
        l = a;
        int h = b;
        while (l < h) {
            const int mid = (l + h) >> 1;
            if (v.F[mid].x < q.x) l = mid + 1; else h = mid;
        }
        start = l;
    }
    // the next record is read while the current one is processed (clamped: always in the strip)
    if (l < b) {
        float4 pn = v.F[l];
        for (int c = l; c < b; ++c) {
            const float4 p = pn;
            pn = v.F[min(c + 1, b - 1)];
            const float dx = q.x - p.x;
            const float t = dx * dx + dy2;
            if (t > bound() || t >= lim) break;
            body(p);
        }
    }
    if (l > a) {
        float4 pn = v.F[l - 1];
        for (int c = l - 1; c >= a; --c) {
            const float4 p = pn;
            pn = v.F[max(c - 1, a)];
            const float dx = q.x - p.x;
            const float t = dx * dx + dy2;
            if (t > bound() || t >= lim) break;
            body(p);
        }
    }
}

// The 1-m region: the query's strip and its neighbour on each side (strips are wider than 1 m).
// pos: the start positions in the query's strip (its own) and the neighbours (-1 until found).
constexpr int kPos1m = 3;
template <class Bound, class Body>
SSF_DEV void visit_1m(const StripView<false>& v, const StripLds& T, const StripGeo& g, int (&pos)[kPos1m],
                      const float4& q, Bound&& bound, Body&& body) {
    const int s0 = g.strip_of(q.y);
    strip_visit(v, T, s0, pos[0], q, 1.0f, bound, body);
    if (s0 + 1 < g.ns) strip_visit(v, T, s0 + 1, pos[1], q, 1.0f, bound, body);
    if (s0 - 1 >= 0) strip_visit(v, T, s0 - 1, pos[2], q, 1.0f, bound, body);
}

// Every strip outward from q's, in rings of strips, while a strip can still hold a point with
// d2 <= bound(): strip s0 +- r has |dy| >= (r - 1) W (less strip_slack, reg_strips.hpp).
template <class Bound, class Body>
SSF_DEV void visit_all(const StripView<false>& v, const StripLds& T, const StripGeo& g, int self, const float4& q,
                       Bound&& bound, Body&& body) {
    const float inf = __builtin_inff();
    const int s0 = g.strip_of(q.y);
    int p0 = self;
    const float slack = strip_slack(g.span(), q.y);
    strip_visit(v, T, s0, p0, q, inf, bound, body);
    for (int r = 1; r < g.ns; ++r) {
        const float lb = (float)(r - 1) * g.W - slack;
        if (lb > 0.0f && lb * lb > bound()) break;
        int pu = -1, pd = -1;
        if (s0 + r < g.ns) strip_visit(v, T, s0 + r, pu, q, inf, bound, body);
        if (s0 - r >= 0) strip_visit(v, T, s0 - r, pd, q, inf, bound, body);
    }
}

// The plane of the five picked points: plane_from_knn from the least-squares solve on
// (identical arithmetic).
SSF_DEV void plane_from_pick(const float4* __restrict__ P, const int (&v5)[5], float plane_max, float nrm[3],
                             uint8_t& ok) {
    float Am[3][5];
    float pts[5][3];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const float4 p = P[v5[j]];
        pts[j][0] = p.x; pts[j][1] = p.y; pts[j][2] = p.z;
        Am[0][j] = p.x; Am[1][j] = p.y; Am[2][j] = p.z;
    }
    qr_solve_5x3(Am, nrm);                                             // :219
    float z = nrm[0] * nrm[0] + nrm[1] * nrm[1];
    z = z + nrm[2] * nrm[2];
    if (z > 0.0f) {                                                    // :220
        const float sq = sqrtf(z);
        nrm[0] = nrm[0] / sq; nrm[1] = nrm[1] / sq; nrm[2] = nrm[2] / sq;
    }
    ok = 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                      // :222-232
        const double vx = (double)(pts[k][0] - pts[k + 1][0]);
        const double vy = (double)(pts[k][1] - pts[k + 1][1]);
        const double vz = (double)(pts[k][2] - pts[k + 1][2]);
        double dd = (double)nrm[0] * vx + (double)nrm[1] * vy;
        dd = dd + (double)nrm[2] * vz;
        if (fabs(dd) > (double)plane_max) { ok = 0; break; }
    }
}

struct PickState {
    int pos[kPos1m];    // strip start positions of the 1-m region (visit_1m)
    double t5[5];       // ranks 0..4
    double d1, d2;      // the first two other-ring keys of rank >= 5 within 1 m (sentinel: 1 m)
    int K1, prow;
    int sl;             // keys that left the top five and are not other-ring (an upper bound
                        // when d1 / d2 come from the second walk: then 1 << 30)
};

// Inside 1 m for query j, one walk: K1, the top five, and the six smallest keys of points on
// another ring than the query's own (at most four of them can be in the top five, so D1 / D2 are
// the first two of them above rank 4).  prow is the ring of rank 0: the query itself unless an
// exact duplicate with a lower index precedes it -- then a second walk with that ring.
SSF_DEV void pick_1m(const float4* __restrict__ P, const StripView<false>& v, const StripLds& T, const StripGeo& g,
                     int j, const float4& q, PickState& s) {
    const double sent = knn_key(1.0f, 0x7fffffff);
#pragma unroll
    for (int k = 0; k < 5; ++k) s.t5[k] = sent;
    // o2: the two smallest other-ring keys that LEFT the top five.  Every key within 1 m either
    // ends in the final top five or leaves it exactly once (the list only improves), so the keys
    // that left are exactly those above the final rank-4 key: o2 = D1, D2 (when rank 0's ring is
    // the query's own; otherwise the second walk below)
    double o2[2] = {sent, sent};
    const int qrow = pt_row(q);
    int K1 = 0, sl = 0;
    s.pos[0] = j;
#pragma unroll
    for (int k = 1; k < kPos1m; ++k) s.pos[k] = -1;
    visit_1m(v, T, g, s.pos, q, [] { return 1.0f; }, [&](const float4& p) {
        const float d = l2_simple(q, p);
        if (d < 1.0f) {
            ++K1;
            const double out = key_insert_out<5>(s.t5, pick_key(d, p));
            const int row = pick_row(out);
            if (row != qrow && row <= 63) key_insert<2>(o2, out);
            else ++sl;
        }
    });
    s.K1 = K1;
    s.sl = 1 << 30;
    s.d1 = sent; s.d2 = sent;
    s.prow = -1;
    if (K1 <= 5) return;
    s.prow = pick_row(s.t5[0]);                                        // row_of(P[rank 0].w)
    const double k5 = s.t5[4];
    if (pick_index(s.t5[0]) == pt_id(q) || s.prow == qrow) {
        s.d1 = o2[0]; s.d2 = o2[1];
        s.sl = sl;
        return;
    }
    const int prow = s.prow;
    double dd[2] = {sent, sent};
    visit_1m(v, T, g, s.pos, q, [&] { return key_dist(dd[1]); }, [&](const float4& p) {
        const float d = l2_simple(q, p);
        const int row = pt_row(p);
        const double key = pick_key(d, p);
        if (d < 1.0f && key > k5 && row != prow && row <= 63) key_insert<2>(dd, key);
    });
    s.d1 = dd[0]; s.d2 = dd[1];
}

SSF_DEV void pick_finish(const float4* __restrict__ P, const PickState& s, int nvr, float plane_max, int64_t o,
                         float* __restrict__ normal, uint8_t* __restrict__ valid) {
    int v5[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) v5[k] = pick_index(s.t5[k]);
    if (nvr == 1) v5[4] = pick_index(s.d1);                            // :199-205
    if (nvr == 2) { v5[3] = pick_index(s.d1); v5[4] = pick_index(s.d2); }
    float nrm[3];
    uint8_t ok;
    plane_from_pick(P, v5, plane_max, nrm, ok);
    normal[3 * o] = nrm[0]; normal[3 * o + 1] = nrm[1]; normal[3 * o + 2] = nrm[2];
    valid[o] = ok;
}

SSF_DEV void pick_invalid(int64_t o, float* __restrict__ normal, uint8_t* __restrict__ valid) {
    normal[3 * o] = 0.f; normal[3 * o + 1] = 0.f; normal[3 * o + 2] = 0.f;
    valid[o] = 0;
}

// Beyond 1 m (K1 < 30, fewer than two other-ring points inside): invalid iff E, the smallest
// key of an other-ring point beyond 1 m, has fewer than 30 - K1 keys beyond 1 m below it.
SSF_DEV bool pick_beyond_invalid(const StripView<false>& v, const StripLds& T, const StripGeo& g, int j,
                                 const float4& q, const PickState& s) {
    double E = knn_key(__builtin_inff(), 0x7fffffff);
    const int prow = s.prow;
    visit_all(v, T, g, j, q, [&] { return key_dist(E); }, [&](const float4& p) {
        const float d = l2_simple(q, p);
        const int row = pt_row(p);
        const double key = pick_key(d, p);
        if (d >= 1.0f && row != prow && row <= 63 && key < E) E = key;
    });
    if (!(key_dist(E) < __builtin_inff())) return false;          // no other-ring point at all
    int C = 0;
    const int need = 30 - s.K1;
    const float lim = key_dist(E);
    visit_all(v, T, g, j, q, [&] { return C >= need ? -1.0f : lim; }, [&](const float4& p) {
        const float d = l2_simple(q, p);
        C += (d >= 1.0f && pick_key(d, p) < E);
    });
    return C < need;
}

constexpr int kTableCoopG = 4;                   // lanes per deferred pick query
// Whole work-group: every query of the frame (m > 30, every ring code < 255).  Queries that need
// points beyond 1 m (K1 < 30, fewer than two other-ring points inside) are queued and finished
// afterwards, spread over the waves.
SSF_DEV void table_pick_walks(const float4* __restrict__ P, const StripView<false>& v, const StripLds& T,
                              const StripGeo& g, int m, float plane_max, int64_t base, float* __restrict__ normal,
                              uint8_t* __restrict__ valid, int* queue, int qcap, int* qlen,
                              int32_t* stamp_out = nullptr, unsigned long long stamp0 = 0,
                              int share = 0, int nshare = 1) {
    // queries of this work-group's share: every nshare-th one (k_plane_table_sorted splits a
    // frame's queries over nshare work-groups for small batches)
    for (int j = share + nshare * (int)threadIdx.x; j < m; j += nshare * (int)blockDim.x) {
        const float4 q = v.pt(j);
        const int64_t o = base + v.id(j);
        PickState s;
        pick_1m(P, v, T, g, j, q, s);
        if (s.K1 <= 5) { pick_invalid(o, normal, valid); continue; }
        const bool f1 = key_dist(s.d1) < 1.0f, f2 = key_dist(s.d2) < 1.0f;
        if (s.K1 >= 30) {
            int r1 = 0, r2 = 0;                                            // ranks of D1, D2
            // the keys below D2 are the top five, D1 and left keys that are not other-ring (D1 /
            // D2 are the two smallest other-ring keys that left): with L such keys r1 <= 5 + L,
            // r2 <= 6 + L, so L <= 23 puts both inside the 30 without the rank walk.  sl = L + 5
            // (the five sentinels left the list too: K1 >= 30)
            if (f1 && s.sl > 28) {
                const double b1 = s.d1, b2 = s.d2;
                const float lim = f2 ? key_dist(b2) : key_dist(b1);
                visit_1m(v, T, g, s.pos, q, [&] { return lim; }, [&](const float4& p) {
                    const double key = pick_key(l2_simple(q, p), p);
                    r1 += key < b1;
                    r2 += key < b2;
                });
            }
            const int nvr = (f1 && r1 < 30) + (f2 && r2 < 30);
            pick_finish(P, s, nvr, plane_max, o, normal, valid);
        } else if (f2) {
            pick_finish(P, s, 2, plane_max, o, normal, valid);
        } else {
            const int slot = atomicAdd(qlen, 1);
            if (slot < qcap) { queue[slot] = j; continue; }
            if (pick_beyond_invalid(v, T, g, j, q, s)) pick_invalid(o, normal, valid);   // queue full
            else pick_finish(P, s, f1 ? 1 : 0, plane_max, o, normal, valid);
        }
    }
    __syncthreads();
#ifdef SSF_TABLE_STAMPS
    if (threadIdx.x == 0 && stamp_out) { stamp_out[0] = (int32_t)((__builtin_amdgcn_s_memtime() - stamp0) >> 4); stamp_out[1] = *qlen; }
#endif
    const int nq = min(*qlen, qcap);
    // one deferred query per group of kTableCoopG lanes: the group's lanes run the 1-m pick
    // redundantly (same bits), then both beyond-1-m searches of pick_beyond_invalid with the
    // strips of each ring round one per lane (strip i of the round order s0, s0+1, s0-1, s0+2,
    // ...), the group's minimum E / sum C after each round -- a lane alone would walk every ring
    // (the slowest deferred query then sets the frame's time: ~0.127 M of ~0.60 M cycles, r03 stamps)
    constexpr int G = kTableCoopG;
    const int gl = threadIdx.x % G, ng = blockDim.x / G;
    for (int k = threadIdx.x / G; k < nq; k += ng) {
        const int j = queue[k];                                       // uniform per group
        const float4 q = v.pt(j);
        const int64_t o = base + v.id(j);
        PickState s;
        pick_1m(P, v, T, g, j, q, s);
        const bool f1 = key_dist(s.d1) < 1.0f;
        const int prow = s.prow, s0 = g.strip_of(q.y), nstrip = 2 * g.ns;   // round order
        const float slack = strip_slack(g.span(), q.y);
        auto strip_at = [&](int i) { return i == 0 ? s0 : ((i & 1) ? s0 + (i + 1) / 2 : s0 - i / 2); };
        auto ring_at = [&](int i) { return (i + 1) / 2; };
        // E: the smallest key of an other-ring point beyond 1 m
        double E = knn_key(__builtin_inff(), 0x7fffffff);
        for (int i0 = 0; i0 < nstrip; i0 += G) {
            // a round's strips all have rings >= ring_at(i0): their |dy| >= (r - 1) W - slack
            const float lb = (float)(ring_at(i0) - 1) * g.W - slack;
            if (i0 > 0 && lb > 0.0f && lb * lb > key_dist(E)) break;   // uniform per group
            const int i = i0 + gl, sidx = strip_at(i);
            if (i < nstrip && sidx >= 0 && sidx < g.ns) {
                int st = sidx == s0 ? j : -1;
                strip_visit(v, T, sidx, st, q, __builtin_inff(), [&] { return key_dist(E); },
                            [&](const float4& p) {
                                const float d = l2_simple(q, p);
                                const int row = pt_row(p);
                                const double key = pick_key(d, p);
                                if (d >= 1.0f && row != prow && row <= 63 && key < E) E = key;
                            });
            }
#pragma unroll
            for (int x = G / 2; x >= 1; x >>= 1) {
                const double y = __shfl_xor(E, x, kWave);
                E = y < E ? y : E;
            }
        }
        bool inval = false;
        if (key_dist(E) < __builtin_inff()) {
            // C: keys beyond 1 m below E; invalid iff C < 30 - K1
            const int need = 30 - s.K1;
            const float lim = key_dist(E);
            int C = 0;
            for (int i0 = 0; i0 < nstrip; i0 += G) {
                const float lb = (float)(ring_at(i0) - 1) * g.W - slack;
                if (C >= need || (i0 > 0 && lb > 0.0f && lb * lb > lim)) break;   // uniform per group
                const int i = i0 + gl, sidx = strip_at(i);
                int c = 0;
                if (i < nstrip && sidx >= 0 && sidx < g.ns) {
                    int st = sidx == s0 ? j : -1;
                    strip_visit(v, T, sidx, st, q, __builtin_inff(), [&] { return lim; },
                                [&](const float4& p) {
                                    const float d = l2_simple(q, p);
                                    c += (d >= 1.0f && pick_key(d, p) < E);
                                });
                }
#pragma unroll
                for (int x = G / 2; x >= 1; x >>= 1) c += __shfl_xor(c, x, kWave);
                C += c;
            }
            inval = C < need;
        }
        if (gl == 0) {
            if (inval) pick_invalid(o, normal, valid);
            else pick_finish(P, s, f1 ? 1 : 0, plane_max, o, normal, valid);
        }
    }
#ifdef SSF_TABLE_STAMPS
    __syncthreads();
    if (threadIdx.x == 0 && stamp_out) stamp_out[4] = (int32_t)((__builtin_amdgcn_s_memtime() - stamp0) >> 4);
#endif
}

// The deferred few (no decision inside 1 m: sparse, far regions) walk the x-sorted copy the
// sort left in global memory (SP / SI, L2-resident), unbounded, from their x rank (binary
// search on (x, index)): a strip ring search there would need a loop nest whose register
// pressure spills the bounded walks that share the kernel.
template <bool kSoa>
SSF_DEV void table_strip_walks(const float4* __restrict__ P, const StripView<kSoa>& v,
                               const StripLds& T, const StripGeo& g, int m, float plane_max,
                               int64_t base, float* __restrict__ normal, uint8_t* __restrict__ valid,
                               int* queue, int qcap, int* qlen, const float4* __restrict__ SP,
                               const int32_t* __restrict__ SI, int32_t* stamp_out,
                               unsigned long long stamp0, int share = 0, int nshare = 1) {
    for (int j = share + nshare * (int)threadIdx.x; j < m; j += nshare * (int)blockDim.x) {
        const float4 q = v.pt(j);
        double kk[kK];
        int dec;
        strip_knn_radius<1>(v, T, g, j, q, kk);
        dec = bounded_decides(P, m, kk);
        if (dec == 0) {
            const int slot = atomicAdd(qlen, 1);
            if (slot < qcap) queue[slot] = j;
            else { table_deferred_walk(P, SP, SI, m, v.id(j), q, kk); dec = 1; }   // queue full
        }
        if (dec == 2) {
            const int64_t o = base + v.id(j);
            normal[3 * o] = 0.f; normal[3 * o + 1] = 0.f; normal[3 * o + 2] = 0.f;
            valid[o] = 0;
        } else if (dec == 1) {
            table_finish(P, m, plane_max, base + v.id(j), kk, normal, valid);
        }
    }
    __syncthreads();
#ifdef SSF_TABLE_STAMPS
    if (threadIdx.x == 0 && stamp_out) { stamp_out[0] = (int32_t)((__builtin_amdgcn_s_memtime() - stamp0) >> 4); stamp_out[1] = *qlen; }
#endif
    const int nq = min(*qlen, qcap);
    // spread the deferred queries over the waves (entry k -> wave k % nw)
    const int nw = blockDim.x >> 6, t2 = (threadIdx.x & 63) * nw + (threadIdx.x >> 6);
    for (int k = t2; k < nq; k += blockDim.x) {
        const int j = queue[k];
        const float4 q = v.pt(j);
        double kk[kK];
        // within 2 m, then within kDeferRings m, from the strips: decided as soon as the exact
        // part of the list settles it (deferred_decides); else the x-sorted global copy, unbounded
        strip_knn_radius<kDeferFirst>(v, T, g, j, q, kk);
        int dec = deferred_decides(P, kk, (float)(kDeferFirst * kDeferFirst));
        if (dec == 0) {
            strip_knn_radius<kDeferRings>(v, T, g, j, q, kk);
            dec = deferred_decides(P, kk, (float)(kDeferRings * kDeferRings));
        }
        if (dec == 0) table_deferred_walk(P, SP, SI, m, v.id(j), q, kk);
        const int64_t o = base + v.id(j);
        if (dec == 2) {
            normal[3 * o] = 0.f; normal[3 * o + 1] = 0.f; normal[3 * o + 2] = 0.f;
            valid[o] = 0;
        } else {
            table_finish(P, m, plane_max, o, kk, normal, valid);
        }
    }
}

// The (x, index) bitonic sort of k_plane_table_sorted with each thread's E elements in registers
// (element t = e kTableThreads + tid): partners 64 <= j < kTableThreads apart go through LDS (one
// barrier per half-stage), j < 64 through wave shuffles, j >= kTableThreads within the thread.
// The same comparator network as the LDS loop (same pairs, directions and comparisons), so the
// same permutation for any input.  Leaves the sorted indices in idx[].
template <int E>
SSF_DEV void table_sort_regs(const float4* __restrict__ P, int m, float* key, int* idx) {
    constexpr int NT = kTableThreads, NP = E * NT;
    const int tid = threadIdx.x;
    float k[E];
    int ix[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int t = e * NT + tid;
        k[e] = t < m ? P[t].x : __builtin_inff();
        ix[e] = t;
    }
    for (int kk = 2; kk <= NP; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            if (j >= NT) {                                          // partner in this thread
                const int je = j / NT;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int e2 = e ^ je;
                    if (e2 > e) {
                        const int t = e * NT + tid;
                        const bool asc = (t & kk) == 0;
                        const bool sw = asc ? lex_less(k[e2], ix[e2], k[e], ix[e]) : lex_less(k[e], ix[e], k[e2], ix[e2]);
                        if (sw) {
                            const float tk = k[e]; k[e] = k[e2]; k[e2] = tk;
                            const int ti = ix[e]; ix[e] = ix[e2]; ix[e2] = ti;
                        }
                    }
                }
            } else if (j >= 64) {                                   // partner in another wave
#pragma unroll
                for (int e = 0; e < E; ++e) { key[e * NT + tid] = k[e]; idx[e * NT + tid] = ix[e]; }
                __syncthreads();
                const bool lower = (tid & j) == 0;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int t = e * NT + tid;
                    const float pk = key[t ^ j];
                    const int pi = idx[t ^ j];
                    const bool asc = (t & kk) == 0;
                    const bool take = (lower == asc) ? lex_less(pk, pi, k[e], ix[e]) : lex_less(k[e], ix[e], pk, pi);
                    if (take) { k[e] = pk; ix[e] = pi; }
                }
                __syncthreads();
            } else {                                                // partner in this wave
                const bool lower = (tid & j) == 0;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int t = e * NT + tid;
                    const float pk = __shfl_xor(k[e], j, 64);
                    const int pi = __shfl_xor(ix[e], j, 64);
                    const bool asc = (t & kk) == 0;
                    const bool take = (lower == asc) ? lex_less(pk, pi, k[e], ix[e]) : lex_less(k[e], ix[e], pk, pi);
                    if (take) { k[e] = pk; ix[e] = pi; }
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) { key[e * NT + tid] = k[e]; idx[e * NT + tid] = ix[e]; }
    __syncthreads();
}

// The same (x, index) order by a stable LSD radix sort of the x bits (rocPRIM
// block_radix_sort, keys and the index in registers, E per thread in blocked order, so equal
// keys keep index order): x + 0 turns -0 into +0 (lex_less compares them equal), the sign-flip
// encoding orders the floats as unsigned words, and slots past m take the largest key.
template <int E>
SSF_DEV void table_sort_radix(const float4* __restrict__ P, int m, void* storage, int* idx) {
    using Sort = rocprim::block_radix_sort<unsigned int, kTableThreads, E, int>;
    // the exchange storage lives in the key region; the index stores below follow the sort with
    // no barrier, so the storage must not reach the index region
    static_assert(sizeof(typename Sort::storage_type) <= kSortMax * 4, "radix sort storage exceeds the key region");
    auto& st = *reinterpret_cast<typename Sort::storage_type*>(storage);
    const int tid = threadIdx.x;
    unsigned int k[E];
    int ix[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int t = tid * E + e;
        const unsigned int b = __float_as_uint(t < m ? P[t].x + 0.0f : 0.0f);
        k[e] = t < m ? (b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u)) : 0xFFFFFFFFu;
        ix[e] = t;
    }
    Sort().sort(k, ix, st);
#pragma unroll
    for (int e = 0; e < E; ++e) idx[tid * E + e] = ix[e];
    __syncthreads();
}

__global__ __launch_bounds__(kTableThreads) void k_plane_table_sorted(
    const float4* __restrict__ plane, const int64_t* __restrict__ frame_off,
    const int32_t* __restrict__ count, float plane_max, float* __restrict__ normal,
    uint8_t* __restrict__ valid, float4* __restrict__ sorted_xyzi, int32_t* __restrict__ sorted_idx,
    float4* __restrict__ strip_xyzi, int32_t* __restrict__ strip_head) {
    // 160 KiB of LDS: [0, 64K) keys, [64K, 128K) permutation, [128K, 160K) spare.  After the
    // sort, frames <= kTableStripSoaMax rebuild the whole image as y-strips of the sorted points
    // + the strip table + the deferred queue; larger frames walk the sorted copy in global memory.
    __shared__ __attribute__((aligned(16))) char lds[kSortMax * 8 + 32768];
    float* key = reinterpret_cast<float*>(lds);
    int* idx = reinterpret_cast<int*>(lds + kSortMax * 4);
    const int f = blockIdx.x, tid = threadIdx.x;
    // small batches: gridDim.y work-groups per frame, each sorting and building the strips
    // (identical results) and walking every gridDim.y-th query; share 0 alone
    // writes the strip image and the stamps (every share writes the sorted copy, see below)
    const int share = (int)blockIdx.y, nshare = (int)gridDim.y;
    const int m = count[f];
    const int64_t base = frame_off[f];
    const float4* P = plane + base;
    if (m <= 0) return;
    if (share > 0 && (m > kTableStripSoaMax || m <= share)) return;   // uniform: no queries here
#ifdef SSF_TABLE_STAMPS
    const unsigned long long tstamp0 = __builtin_amdgcn_s_memtime();
#endif
    int np = 1;
    while (np < m) np <<= 1;
    // the key region [0, 64 KiB) holds the radix sort's storage (the keys stay in registers)
    if (np <= kTableThreads) table_sort_radix<1>(P, m, lds, idx);
    else if (np == 2 * kTableThreads) table_sort_radix<2>(P, m, lds, idx);
    else if (np == 4 * kTableThreads) table_sort_radix<4>(P, m, lds, idx);
    else if (np == 8 * kTableThreads) table_sort_radix<8>(P, m, lds, idx);
    else if (np == 16 * kTableThreads) table_sort_regs<16>(P, m, key, idx);
    else {
    for (int r = tid; r < np; r += blockDim.x) {
        key[r] = r < m ? P[r].x : __builtin_inff();
        idx[r] = r;
    }
    __syncthreads();
    for (int k = 2; k <= np; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < np; t += blockDim.x) {
                const int u = t ^ j;
                if (u > t) {
                    const float ka = key[t], kb = key[u];
                    const int ia = idx[t], ib = idx[u];
                    const bool asc = (t & k) == 0;
                    if (asc ? lex_less(kb, ib, ka, ia) : lex_less(ka, ia, kb, ib)) {
                        key[t] = kb; key[u] = ka; idx[t] = ib; idx[u] = ia;
                    }
                }
            }
            __syncthreads();
        }
    }
    }
    float4* SP = sorted_xyzi + base;
    int32_t* SI = sorted_idx + base;
    // EVERY share writes the sorted copy: table_strip_walks' deferred walk reads it back
    // (table_deferred_walk), and only this work-group's own stores are ordered before those reads
    // by the barrier below -- another share's (possibly on another XCD, whose L2 is not coherent
    // for plain stores) are not.  The shares write identical values, so the duplicates are benign.
    for (int r = tid; r < m; r += blockDim.x) {
        SP[r] = P[idx[r]];
        SI[r] = idx[r];
    }
    __syncthreads();
    SSF_TSTAMP(0);
    int* qlen = reinterpret_cast<int*>(lds + sizeof(lds) - 4);   // last word of the LDS image
    if (tid == 0) *qlen = 0;
    if (m <= kTableStripSoaMax) {
        // the sorted permutation into registers (the strip layout overwrites the sort image),
        // then the strip-major points, the strip table and the deferred queue in the 160 KiB
        const bool soa = m > kTableStripF4Max;                          // uniform
        int own[kStripPerMax];
#pragma unroll
        for (int k = 0; k < kStripPerMax; ++k) {
            const int r = k * kTableThreads + tid;
            own[k] = r < m ? idx[r] : 0;
        }
        __syncthreads();
        float4* F = reinterpret_cast<float4*>(lds);
        float* X = reinterpret_cast<float*>(lds);
        uint16_t* I16 = reinterpret_cast<uint16_t*>(X + 3 * m);
        const int toff = ((soa ? 14 * m : 16 * m) + 15) & ~15;
        StripLds& T = *reinterpret_cast<StripLds*>(lds + toff);
        const int qoff = (toff + (int)sizeof(StripLds) + 15) & ~15;
        int* queue = reinterpret_cast<int*>(lds + qoff);
        const int qcap = ((int)sizeof(lds) - 4 - qoff) / 4;
        auto get = [&](int k, int) {
            float4 p = P[own[k]];
            p.w = __int_as_float(own[k]);
            return p;
        };
#ifdef SSF_TABLE_STAMPS
        int32_t* stamp_out = share == 0 ? SI + m + 1 : nullptr;
        const unsigned long long st0 = tstamp0;
#else
        int32_t* stamp_out = nullptr;
        const unsigned long long st0 = 0;
#endif
#ifdef SSF_TABLE_STAMPS
#define SSF_TSTAMP_BUILD() do { if (tid == 0 && stamp_out) stamp_out[3] = (int32_t)((__builtin_amdgcn_s_memtime() - st0) >> 4); } while (0)
#else
#define SSF_TSTAMP_BUILD() do { } while (0)
#endif
        if (soa) {
            const StripGeo g = strips_build<true, kStripPerMax>(get, m, T, F, X, I16);
            SSF_TSTAMP_BUILD();
            table_strip_walks(P, StripView<true>{F, X, I16, m}, T, g, m, plane_max, base, normal,
                              valid, queue, qcap, qlen, SP, SI, stamp_out, st0, share, nshare);
        } else {
            // 16-B records carry the ring code of every point (bits 16..23 of .w): the pick then
            // runs without the 30-key list (table_pick_walks) unless the frame is tiny or a ring
            // code is out of range (intensities frameFeature never writes)
            bool rows_ok = true;
#pragma unroll
            for (int k = 0; k < kStripPerMax; ++k) {
                const int r = k * kTableThreads + tid;
                if (r < m) rows_ok = rows_ok && row_code(P[own[k]].w) != kRowCodeBad;
            }
            int* rflag = reinterpret_cast<int*>(lds + sizeof(lds) - 8);   // next to qlen, free here
            if (tid == 0) *rflag = 1;
            __syncthreads();
            if (!rows_ok) *rflag = 0;
            __syncthreads();
            rows_ok = *rflag != 0;
            auto getp = [&](int k, int) {
                float4 p = P[own[k]];
                p.w = __int_as_float(own[k] | (int)(row_code(p.w) << 16));
                return p;
            };
            const bool pick = rows_ok && m > kK;                            // uniform
            const StripGeo g = strips_build<false, kStripPerMax>(getp, m, T, F, X, I16);
            SSF_TSTAMP_BUILD();
            // results staged in LDS at their original index and stored coalesced at the end when
            // 13 B per point fit behind the strip image with a queue of m / 4 entries (m <= ~5000):
            // scattered 12-B normal and 1-B validity stores each cost a 64-B write request
            const int soff = ((int)sizeof(lds) - 16 - 13 * m) & ~15;
            // (one work-group per frame only: a share's results are scattered over the frame)
            const bool stage = nshare == 1 && (soff - qoff) / 4 >= m / 4 + 64;   // uniform
            if (pick && stage) {
                float* nl = reinterpret_cast<float*>(lds + soff);
                uint8_t* vl = reinterpret_cast<uint8_t*>(lds + soff + 12 * m);
                table_pick_walks(P, StripView<false>{F, X, I16, m}, T, g, m, plane_max, 0, nl, vl,
                                 queue, (soff - qoff) / 4, qlen, stamp_out, st0);
                __syncthreads();
                float* gn = normal + 3 * base;
                uint8_t* gv = valid + base;
                for (int k = tid; k < 3 * m; k += kTableThreads) gn[k] = nl[k];
                for (int k = tid; k < m; k += kTableThreads) gv[k] = vl[k];
            } else if (pick)
                table_pick_walks(P, StripView<false>{F, X, I16, m}, T, g, m, plane_max, base, normal, valid,
                                 queue, qcap, qlen, stamp_out, st0, share, nshare);
            else
                table_strip_walks(P, StripView<false>{F, X, I16, m}, T, g, m, plane_max, base, normal,
                                  valid, queue, qcap, qlen, SP, SI, stamp_out, st0, share, nshare);
            // the walks only read F and T: the image leaves as it is (uniform condition)
            if (share == 0 && strip_xyzi && strip_image_frame(m))
                strip_image_store(F, T, g, m, strip_xyzi + base, strip_head + base);
        }
        SSF_TSTAMP(3);
    } else {
        // points from global memory, the permutation in LDS; queue in the (now unused) key region
        int* queue = reinterpret_cast<int*>(lds);
        const PtsF4 v{SP, idx};
        table_walks(P, v, m, plane_max, base, normal, valid, queue, kSortMax, qlen);
    }
}

__global__ __launch_bounds__(256) void k_strip_invalidate(const int64_t* __restrict__ frame_off,
                                                          const int32_t* __restrict__ count, int n_frames,
                                                          int32_t* __restrict__ strip_head) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < n_frames && strip_image_frame(count[f])) strip_head[frame_off[f] + 3 * kStripMax + 4] = 0;
}

hipError_t launch_plane_table(hipStream_t s, const ssf_config& cfg, int n_frames,
                              const float4* plane, const int64_t* frame_off, const int32_t* count,
                              int64_t max_m, float* normal, uint8_t* valid, float4* sorted_xyzi,
                              int32_t* sorted_idx, float4* strip_xyzi, int32_t* strip_head) {
    if (n_frames <= 0 || max_m <= 0) return hipSuccess;
    if (max_m <= kSortMax && sorted_xyzi && sorted_idx) {
        // few frames (a node's one frame, configs[2]'s 32): up to 8 work-groups per frame share
        // its queries (each sorts and builds the strips itself), so the launch spreads over the
        // chip instead of n_frames CUs; 256 frames and more keep one work-group per frame
        const int qsplit = (int)std::max<int64_t>(1, std::min<int64_t>({SSF_TABLE_MAX_SPLIT, 256 / n_frames,
                                                             max_m / 256}));
        kmark(s, "k_plane_table_sorted");
        hipLaunchKernelGGL(k_plane_table_sorted, dim3(n_frames, qsplit), dim3(kTableThreads), 0, s, plane,
                           frame_off, count, cfg.plane_max, normal, valid, sorted_xyzi, sorted_idx,
                           strip_head ? strip_xyzi : nullptr, strip_head);
    } else {
        const int bx = (int)((max_m + 255) / 256);
        kmark(s, "k_plane_table");
        hipLaunchKernelGGL(k_plane_table, dim3(bx, n_frames), dim3(256), 0, s, plane, frame_off,
                           count, cfg.plane_max, normal, valid);
        if (strip_head)                     // no image from this launch: no frame may look imaged
            hipLaunchKernelGGL(k_strip_invalidate, dim3((n_frames + 255) / 256), dim3(256), 0, s,
                               frame_off, count, n_frames, strip_head);
    }
    return hipGetLastError();
}

}  // namespace ssf
