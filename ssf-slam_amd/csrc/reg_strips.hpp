// reg_strips.hpp -- the y-strip layout of an x-sorted plane cloud and its size limits, shared by
// the sorted plane table (plane_table.hip), which builds the strips and keeps their image, and
// the strip association (associate.hip), which stages that image or builds the strips itself.
#pragma once
#include "reg_knn.hpp"

namespace ssf {

constexpr int kSortMax = 16384;           // plane points per frame sorted in LDS (128 KiB)
constexpr int kTableStripF4Max = 9216;    // after the sort, frames up to this size search strips of
// 16-B points in LDS (16 m + the 12 KiB strip table + >= 2 KiB of deferred queue) ...
constexpr int kTableStripSoaMax = 10624;  // ... and up to this size strips of 14-B SoA points

// Sorted-point views the walks read through (all inlined; the address space of each pointer --
// LDS or global -- is inferred at the call site):
//   PtsF4  16-B points (x, y, z, -) + a separate int permutation (sorted rank -> original index)
struct PtsF4 {
    const float4* S;
    const int* I;
    SSF_DEV float4 pt(int c) const { return S[c]; }
    SSF_DEV int id(int c) const { return I[c]; }
};

// ------------------------------------------------------------------------------------------
// y-strips (shared by the plane table and the association; see k_associate_strips for the
// search and its exactness argument)
constexpr int kStripThreads = 1024;
constexpr int kStripMax = 256;             // strips per frame (W widened beyond 255 m of y)
constexpr int kStripWaves = kStripThreads / 64;
constexpr int kAssocStripF4Max = 6144;     // 16-B points (x, y, z, index) staged: 96 KiB
constexpr int kAssocStripSoaMax = 10752;   // x | y | z + u16 index (14 B): 147 KiB

struct StripLds {
    int start[kStripMax + 1];
    int cursor[kStripMax];
    float ylo[kStripMax], yhi[kStripMax];
    uint16_t wc[kStripWaves][kStripMax];
    float red[2 * kStripWaves];
};

struct StripGeo {
    float y0, W, invW;
    int ns;
    SSF_DEV int strip_of(float y) const { return min(ns - 1, max(0, (int)((y - y0) * invW))); }
    // |y0| + an upper bound of |y1| (|y1| <= |y0| + ns W): the frame's part of strip_slack
    SSF_DEV float span() const { return 2.0f * fabsf(y0) + (float)ns * W; }
};

// Slack of a ring stop: what a search subtracts from a NOMINAL strip distance -- y0 + su W - qy
// (the association's lane mode), (r - 1) W (the plane table's searches beyond 1 m) -- so that it
// stays a lower bound of the float |dy| of every point of the strips it cuts off.  With
// eps = 2^-24: strip_of puts p in a strip >= su when fl(fl(p.y - y0) invW) >= su, three roundings,
// so p.y >= y0 + su W - 3 eps E, E = su W <= the extent (a query of the cloud itself is placed the
// same way: 3 eps E more).  The stop forms fl(y0 + fl(su W)), eps E and eps Y more (Y = max |y|),
// or fl((r - 1) W), eps E; then fl(. - qy) and fl(. - slack), eps (Y + |qy|) each; and the distance
// it must not exceed is built on fl(qy - p.y), one more.  With S = |y0| + |y1| + |qy| >= E and
// >= Y + |qy| that is at most 9 eps S; 16 eps S is taken.  Below S ~ 1 km the slack is the 1 mm
// every scan has always had (no walk of a scan changes); at 30 km of extent it is ~7 cm.
constexpr float kStripSlackMin = 1e-3f;
constexpr float kStripSlackRel = 16.0f * 5.9604645e-8f;            // 16 eps
SSF_DEV float strip_slack(float span, float qy) { return fmaxf(kStripSlackMin, kStripSlackRel * (span + fabsf(qy))); }

// The plane table's strip image, kept for the association of the pairs whose LAST frame it is
// (strips_build is deterministic and both kernels run it on the same x-sorted points with the
// same work-group size, so the image is the one the association would build).  Per frame of
// m points, at the frame's offset: m float4 strip-major points (original index in the low 16
// bits of .w), and kStripHeadWords int32 words {start[kStripMax + 1], ylo[kStripMax],
// yhi[kStripMax], y0, W, invW, ns}.  Frames with kStripHeadWords <= m <= kAssocStripF4Max only
// (the header lives in the frame's own m words; the association stages float4 up to there).
constexpr int kStripHeadWords = (kStripMax + 1) + 2 * kStripMax + 4;
SSF_DEV bool strip_image_frame(int m) { return m >= kStripHeadWords && m <= kAssocStripF4Max; }
// every frame the association may stage from an image is one the table imaged: the table sorts
// it (<= kSortMax) and keeps its float4 strips (<= kTableStripF4Max)
static_assert(kTableStripF4Max >= kAssocStripF4Max && kSortMax >= kAssocStripF4Max,
              "strip image: the table must image every frame the association stages as float4");
// The header's last word is ns | kStripImageMagic << 16; a frame whose table launch did not image
// it carries 0 there (k_plane_table_sorted's other branches, k_strip_invalidate), and the
// association builds its strips itself unless the word checks out.
constexpr int32_t kStripImageMagic = 0x57A1;
SSF_DEV bool strip_image_valid(const int32_t* __restrict__ head) {
    const int32_t v = head[3 * kStripMax + 1 + 3];
    const int ns = v & 0xffff;
    return (v >> 16) == kStripImageMagic && ns >= 1 && ns <= kStripMax;
}

SSF_DEV void strip_image_store(const float4* F, const StripLds& T, const StripGeo& g, int m,
                               float4* __restrict__ img, int32_t* __restrict__ head) {
    for (int r = threadIdx.x; r < m; r += blockDim.x) img[r] = F[r];
    for (int j = threadIdx.x; j <= kStripMax; j += blockDim.x) head[j] = T.start[j];
    for (int j = threadIdx.x; j < g.ns; j += blockDim.x) {
        head[kStripMax + 1 + j] = __float_as_int(T.ylo[j]);
        head[2 * kStripMax + 1 + j] = __float_as_int(T.yhi[j]);
    }
    if (threadIdx.x == 0) {
        int32_t* gh = head + 3 * kStripMax + 1;
        gh[0] = __float_as_int(g.y0); gh[1] = __float_as_int(g.W); gh[2] = __float_as_int(g.invW);
        gh[3] = g.ns | (kStripImageMagic << 16);
    }
}

// The association's side: the image into its LDS (F, T), the geometry returned.
SSF_DEV StripGeo strip_image_load(const float4* __restrict__ img, const int32_t* __restrict__ head, int m,
                                  float4* F, StripLds& T) {
    const int32_t* gh = head + 3 * kStripMax + 1;
    StripGeo g;
    g.y0 = __int_as_float(gh[0]); g.W = __int_as_float(gh[1]); g.invW = __int_as_float(gh[2]); g.ns = gh[3] & 0xffff;
    for (int r = threadIdx.x; r < m; r += blockDim.x) F[r] = img[r];
    for (int j = threadIdx.x; j <= kStripMax; j += blockDim.x) T.start[j] = head[j];
    for (int j = threadIdx.x; j < g.ns; j += blockDim.x) {
        T.ylo[j] = __int_as_float(head[kStripMax + 1 + j]);
        T.yhi[j] = __int_as_float(head[2 * kStripMax + 1 + j]);
    }
    __syncthreads();
    return g;
}

// The strip-major points, either layout: float4 (x, y, z, original index in .w) or x | y | z
// float arrays + a u16 original index.
template <bool kSoa>
struct StripView {
    const float4* F;
    const float* X;
    const uint16_t* I;
    int m;
    SSF_DEV float4 pt(int c) const { return kSoa ? make_float4(X[c], X[m + c], X[2 * m + c], 0.f) : F[c]; }
    SSF_DEV float x(int c) const { return kSoa ? X[c] : F[c].x; }
    SSF_DEV float y(int c) const { return kSoa ? X[m + c] : F[c].y; }
    // 16-B layout: original index in the low 16 bits of .w; the plane table packs the point's
    // ring code (row_code) in bits 16..23
    SSF_DEV int id(int c) const { return kSoa ? (int)I[c] : (__float_as_int(F[c].w) & 0xFFFF); }
};

constexpr int kStripPerMax = kSortMax / kStripThreads;   // x-order points per thread (16)

// Whole work-group (kStripThreads): partition m x-sorted points into y-strips, x order kept in
// each strip (stable: per-wave match masks on the strip id, per-wave strip counts, one chunk of
// kStripThreads points in x order at a time).  get(k, r) returns the point of x-sorted rank
// r = k kStripThreads + tid with its original index in .w.  Writes the strip-major points (F,
// or X | Y | Z + I16), T.start / T.ylo / T.yhi; returns the strip geometry.
template <bool kSoa, int kPer, class Get>
SSF_DEV StripGeo strips_build(Get get, int m, StripLds& T, float4* F, float* X, uint16_t* I16) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float y0 = __builtin_inff(), y1 = -__builtin_inff();
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int r = k * kStripThreads + tid;
        if (r < m) { const float y = get(k, r).y; y0 = fminf(y0, y); y1 = fmaxf(y1, y); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { y0 = fminf(y0, __shfl_xor(y0, o, 64)); y1 = fmaxf(y1, __shfl_xor(y1, o, 64)); }
    if (lane == 0) { T.red[2 * w] = y0; T.red[2 * w + 1] = y1; }
    for (int k = tid; k < kStripWaves * kStripMax; k += kStripThreads) (&T.wc[0][0])[k] = 0;
    for (int k = tid; k < kStripMax; k += kStripThreads) T.cursor[k] = 0;
    __syncthreads();
    StripGeo g;
    y0 = __builtin_inff(); y1 = -__builtin_inff();
    for (int k = 0; k < kStripWaves; ++k) { y0 = fminf(y0, T.red[2 * k]); y1 = fmaxf(y1, T.red[2 * k + 1]); }
    g.y0 = y0;
    // W > 1 m by a margin far above the float error of the strip assignment: a point two strips
    // away from the query's is then always more than 1 m away (the bounded 30-NN and the pick
    // walks search the query's strip and its two neighbours only)
    g.W = fmaxf(1.001f, (y1 - y0) / (float)(kStripMax - 1));
    g.invW = 1.0f / g.W;
    g.ns = min(kStripMax, (int)((y1 - y0) * g.invW) + 1);
    // histogram (cursor holds the counts), exclusive scan into start
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int r = k * kStripThreads + tid;
        if (r < m) atomicAdd(&T.cursor[g.strip_of(get(k, r).y)], 1);
    }
    __syncthreads();
    if (w == 0) {
        constexpr int per = (kStripMax + 63) / 64;                      // 4 strips per lane
        int run = 0;
        for (int k = 0; k < per; ++k) run += T.cursor[lane * per + k];
        int incl = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(incl, o, 64); if (lane >= o) incl += y; }
        int pre = incl - run;
        for (int k = 0; k < per; ++k) {
            const int sidx = lane * per + k;
            T.start[sidx] = pre;
            pre += T.cursor[sidx];
            T.cursor[sidx] = T.start[sidx];
        }
        if (lane == 63) T.start[kStripMax] = incl;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) {                                    // stable scatter by chunk
        if (k * kStripThreads >= m) break;                              // uniform
        const int r = k * kStripThreads + tid;
        const bool v = r < m;
        float4 pt = make_float4(0.f, 0.f, 0.f, 0.f);
        int sidx = 0;
        if (v) { pt = get(k, r); sidx = g.strip_of(pt.y); }
        uint64_t eq = __ballot(v);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const uint64_t bb = __ballot((sidx >> b) & 1);
            eq &= ((sidx >> b) & 1) ? bb : ~bb;
        }
        const int rank = __popcll(eq & lanemask_lt());
        if (v && rank == 0) T.wc[w][sidx] = (uint16_t)__popcll(eq);
        __syncthreads();
        if (v) {
            int before = T.cursor[sidx];
            for (int j = 0; j < w; ++j) before += T.wc[j][sidx];
            const int dst = before + rank;
            if (kSoa) {
                X[dst] = pt.x; X[m + dst] = pt.y; X[2 * m + dst] = pt.z;
                I16[dst] = (uint16_t)__float_as_int(pt.w);
            } else {
                F[dst] = pt;
            }
        }
        __syncthreads();
        for (int j = tid; j < kStripMax; j += kStripThreads) {
            int add = 0;
            for (int u = 0; u < kStripWaves; ++u) { add += T.wc[u][j]; T.wc[u][j] = 0; }
            T.cursor[j] += add;
        }
        __syncthreads();
    }
    // actual y extent of every strip (the in-strip lower bound of |dy|)
    const StripView<kSoa> v{F, X, I16, m};
    for (int j = tid; j < g.ns; j += kStripThreads) {
        float a = __builtin_inff(), b = -__builtin_inff();
        for (int c = T.start[j]; c < T.start[j + 1]; ++c) { const float y = v.y(c); a = fminf(a, y); b = fmaxf(b, y); }
        T.ylo[j] = a; T.yhi[j] = b;
    }
    __syncthreads();
    return g;
}

// One strip of the k-NN search: binary search of q.x (or the query's own position `start`),
// outward walks while fl(dx^2) + fl(dymin^2) can still beat the 30th key and stays below lim.
template <bool kSoa>
SSF_DEV void strip_search(const StripView<kSoa>& v, const StripLds& T, int sidx, int start,
                          const float4& q, float lim, double (&kk)[kK]) {
    const int a = T.start[sidx], b = T.start[sidx + 1];
    if (a >= b) return;
    const float yl = T.ylo[sidx], yh = T.yhi[sidx];
    const float dyl = q.y < yl ? yl - q.y : (q.y > yh ? q.y - yh : 0.0f);
    const float dy2 = dyl * dyl;
    if (dy2 > key_dist(kk[kK - 1]) || dy2 >= lim) return;
    int l = start;
    if (l < 0) {
        l = a;
        int h = b;                                                       // first x >= q.x
        while (l < h) {
            const int mid = (l + h) >> 1;
            if (v.x(mid) < q.x) l = mid + 1; else h = mid;
        }
    }
    for (int c = l; c < b; ++c) {                                        // rightwards
        const float4 p = v.pt(c);
        const float dx = q.x - p.x;
        const float t = dx * dx + dy2;
        if (t > key_dist(kk[kK - 1]) || t >= lim) break;
        key_insert<kK>(kk, knn_key(l2_simple(q, p), v.id(c)));
    }
    for (int c = l - 1; c >= a; --c) {                                   // leftwards
        const float4 p = v.pt(c);
        const float dx = q.x - p.x;
        const float t = dx * dx + dy2;
        if (t > key_dist(kk[kK - 1]) || t >= lim) break;
        key_insert<kK>(kk, knn_key(l2_simple(q, p), v.id(c)));
    }
}

// k-NN within radius R = kRings m (keys seeded (R^2, INT_MAX), walks stop at R^2): with
// W > 1 m only the query's strip (searched from its own position) and kRings strips on either
// side can hold points within R.  Keys are (distance, original index), so the list equals the
// x-walk's for every point closer than R; kRings = 1 is knn_walk's 1-m bounded mode.  The
// strips are unrolled (no loop nest around the walks: that spilled the 30 keys).
template <int kRings, bool kSoa>
SSF_DEV void strip_knn_radius(const StripView<kSoa>& v, const StripLds& T, const StripGeo& g,
                              int self, const float4& q, double (&kk)[kK]) {
    constexpr float R2 = (float)(kRings * kRings);
#pragma unroll
    for (int k = 0; k < kK; ++k) kk[k] = knn_key(R2, 0x7fffffff);
    const int s0 = g.strip_of(q.y);
    strip_search(v, T, s0, self, q, R2, kk);
#pragma unroll
    for (int rr = 1; rr <= kRings; ++rr) {
        if (s0 + rr < g.ns) strip_search(v, T, s0 + rr, -1, q, R2, kk);
        if (s0 - rr >= 0) strip_search(v, T, s0 - rr, -1, q, R2, kk);
    }
}

}  // namespace ssf
