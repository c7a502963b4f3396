// scan_context.hip -- place recognition by Scan Context descriptors (Kim & Kim, IROS 2018) for the
// map back-end's loop detection, on gfx950.  The definitions are the project's
// own (include/ssf_frontend.h): a 20 ring x 60 sector polar image of the maximum height above the
// ground, a column-wise cosine distance minimised over the 60 column shifts, and the nearest
// candidate of an eligible prefix of the database in the order (dist, index).
//
// The CPU implementations prune the database with a kd-tree over ring keys and pick the shift
// from sector keys, because one full comparison is 60 x 60 x 20 multiply-adds.  Here every
// candidate is compared at every shift: with the columns normalised the comparison is the Gram
// matrix G = Q^T C (60 x 60, K = 20), four 32 x 32 tiles of the f32 MFMA, and shift s is the mean
// of the wrapped diagonal G[j][(j + s) % 60].
//
//   k_sc_describe  one work-group per cloud: a 1200-bin LDS table, the maximum taken with LDS
//                  integer atomics on the bit pattern of the non-negative height.
//   k_sc_match     one wave per (query, candidate) pair: normalise the candidate's columns on
//                  load, G by MFMA, G parked in LDS, lane s sums its diagonal in the order j = 0..59.
//   k_sc_select    one work-group per query: the smallest (dist, index) of the eligible prefix.
//   k_sc_select_topk  one work-group per query: the K smallest whose indices lie more than an
//                  exclusion window apart, taken greedily in the same order.
//
// Nothing is exchanged between work-groups, there are no global or float atomics and every sum
// has a fixed order: a pair's dist and shift are the same bits whatever else is in the batch.
#include <climits>

#include "ssf_device.hpp"
#include "ssf_internal.hpp"

namespace ssf {

constexpr int kScRings = SSF_SC_RINGS, kScSectors = SSF_SC_SECTORS;
constexpr int kScBins = kScRings * kScSectors;

// ------------------------------------------------------------------------------ descriptor
constexpr int kScDescT = 1024;

__global__ __launch_bounds__(kScDescT) void k_sc_describe(const float* __restrict__ pts, int stride,
                                                          const int64_t* __restrict__ off, float max_range,
                                                          float lidar_height, float* __restrict__ desc) {
    __shared__ uint32_t bins[kScBins];
    const int tid = threadIdx.x;
    const int f = blockIdx.x;
    for (int k = tid; k < kScBins; k += kScDescT) bins[k] = 0u;
    __syncthreads();
    const int64_t b = off[f], e = off[f + 1];
    const float ring_w = max_range / (float)kScRings;
    constexpr float kTwoPi = 6.283185307179586f;
    constexpr float kSectorW = kTwoPi / (float)kScSectors;
#pragma unroll 4
    for (int64_t i = b + tid; i < e; i += kScDescT) {
        const float* p = pts + i * stride;
        const float x = p[0], y = p[1], z = p[2];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) continue;
        const float r = sqrtf(x * x + y * y);
        if (!(r < max_range)) continue;
        const float h = z + lidar_height;
        if (!(h > 0.0f)) continue;                   // max(0, .): the empty bin's value already
        int ring = (int)(r / ring_w);
        ring = ring > kScRings - 1 ? kScRings - 1 : ring;
        float phi = atan2f(y, x);
        if (phi < 0.0f) phi += kTwoPi;
        int sector = (int)(phi / kSectorW);
        sector = sector > kScSectors - 1 ? kScSectors - 1 : (sector < 0 ? 0 : sector);
        // non-negative floats order as their bit patterns; a bin only grows, so a stale read that
        // is already at least h needs no atomic
        const uint32_t bits = __float_as_uint(h);
        uint32_t* slot = &bins[ring * kScSectors + sector];
        if (*(volatile uint32_t*)slot < bits) atomicMax(slot, bits);
    }
    __syncthreads();
    float* out = desc + (int64_t)f * kScBins;
    for (int k = tid; k < kScBins; k += kScDescT) out[k] = __uint_as_float(bins[k]);
}

hipError_t launch_sc_describe(hipStream_t s, int n_clouds, const float* pts, int stride, const int64_t* off,
                              float max_range, float lidar_height, float* desc) {
    if (n_clouds <= 0) return hipSuccess;
    kmark(s, "k_sc_describe");
    hipLaunchKernelGGL(k_sc_describe, dim3(n_clouds), dim3(kScDescT), 0, s, pts, stride, off, max_range,
                       lidar_height, desc);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ distance
constexpr int kScMatchT = 256;                       // four waves, one candidate each at a time
constexpr int kScMatchW = kScMatchT / 64;
constexpr int kScCpw = 4;                            // candidates per wave and work-group
constexpr int kScLd = 64;                            // columns padded to the MFMA tiles
constexpr int kScQFloats = kScRings * kScLd;         // the normalised query, [ring][column]
constexpr int kScWaveFloats = kScLd * kScLd;         // a wave's candidate image, then its G
constexpr size_t kScMatchLds = (size_t)(kScQFloats + kScMatchW * kScWaveFloats) * sizeof(float);
constexpr uint64_t kScMask = (1ull << kScSectors) - 1ull;

typedef float sc_f16v __attribute__((ext_vector_type(16)));

// Lane j < 60 takes column j of a descriptor, scales it to unit length (by its largest bin first,
// so the squares neither underflow nor overflow) and writes it to dst[ring * 64 + j]; an invalid
// column (no bin above 0) and the pad columns 60..63 are written as zero.  -> the validity mask.
SSF_DEV uint64_t sc_load_normalised(const float* __restrict__ d, float* dst, int lane) {
    const bool in = lane < kScSectors;
    float c[kScRings];
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < kScRings; ++k) {
        c[k] = in ? d[k * kScSectors + lane] : 0.0f;
        m = fmaxf(m, c[k]);
    }
    const bool valid = m > 0.0f;
    const float rm = valid ? 1.0f / m : 0.0f;
    float ss = 0.0f;
#pragma unroll
    for (int k = 0; k < kScRings; ++k) {
        c[k] = c[k] * rm;
        ss = ss + c[k] * c[k];
    }
    const float rn = valid ? 1.0f / sqrtf(ss) : 0.0f;
#pragma unroll
    for (int k = 0; k < kScRings; ++k) dst[k * kScLd + lane] = c[k] * rn;
    return __ballot(valid);
}

struct ScMatchArgs {
    const float* query;        // [Q, 20, 60]
    const float* db;           // [N, 20, 60]
    float* dist;               // [Q, n_db]
    int32_t* shift;            // [Q, n_db]
    int n_db;                  // row length of dist / shift
    int n_cols;                // candidates 0 .. n_cols - 1 are compared
    int groups;                // work-groups per query
};

__global__ __launch_bounds__(kScMatchT) void k_sc_match(ScMatchArgs a) {
    extern __shared__ float sc_lds[];
    __shared__ uint64_t qmask_s;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q = (int)(blockIdx.x / (unsigned)a.groups), g = (int)(blockIdx.x % (unsigned)a.groups);
    float* qn = sc_lds;
    float* wl = sc_lds + kScQFloats + w * kScWaveFloats;
    if (w == 0) {
        const uint64_t m = sc_load_normalised(a.query + (int64_t)q * kScBins, qn, lane);
        if (lane == 0) qmask_s = m;
    }
    __syncthreads();
    const uint64_t qmask = qmask_s;
    const int r = lane & 31, h = lane >> 5;
    const int base = g * (kScMatchW * kScCpw);
    for (int it = 0; it < kScCpw; ++it) {
        const int c0 = base + it * kScMatchW;        // the same for every wave: the barriers below match
        if (c0 >= a.n_cols) break;
        const int cand = c0 + w;
        const bool active = cand < a.n_cols;
        const uint64_t cmask = sc_load_normalised(a.db + (int64_t)(active ? cand : a.n_cols - 1) * kScBins, wl, lane);
        __syncthreads();
        // G[i][j] = sum_k q[k][i] c[k][j], k ascending.  A: lane l holds A[i = l & 31][k = l >> 5],
        // B: lane l holds B[k = l >> 5][j = l & 31]
        sc_f16v g00, g01, g10, g11;
#pragma unroll
        for (int i = 0; i < 16; ++i) { g00[i] = 0.0f; g01[i] = 0.0f; g10[i] = 0.0f; g11[i] = 0.0f; }
#pragma unroll
        for (int k0 = 0; k0 < kScRings; k0 += 2) {
            const int row = (k0 + h) * kScLd;
            const float qa = qn[row + r], qb = qn[row + 32 + r];
            const float ca = wl[row + r], cb = wl[row + 32 + r];
            g00 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa, ca, g00, 0, 0, 0);
            g01 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa, cb, g01, 0, 0, 0);
            g10 = __builtin_amdgcn_mfma_f32_32x32x2f32(qb, ca, g10, 0, 0, 0);
            g11 = __builtin_amdgcn_mfma_f32_32x32x2f32(qb, cb, g11, 0, 0, 0);
        }
        __syncthreads();
        // park G over the candidate image.  C/D map of the 32x32 MFMA: column = lane & 31,
        // row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
            wl[row * kScLd + r] = g00[i];
            wl[row * kScLd + 32 + r] = g01[i];
            wl[(32 + row) * kScLd + r] = g10[i];
            wl[(32 + row) * kScLd + 32 + r] = g11[i];
        }
        __syncthreads();
        // lane s: the wrapped diagonal of shift s, j ascending (an invalid column is a zero row or
        // column of G, so the sum over all j is the sum over the jointly valid ones)
        const int s = lane < kScSectors ? lane : 0;
        float sum = 0.0f;
        for (int j = 0; j < kScSectors; ++j) {
            int cj = j + s;
            cj = cj >= kScSectors ? cj - kScSectors : cj;
            sum = sum + wl[j * kScLd + cj];
        }
        // bit j of rot: candidate column (j + s) % 60 is valid
        const uint64_t rot = ((cmask >> s) | (cmask << (kScSectors - s))) & kScMask;
        const int cnt = __popcll(qmask & rot);
        float d = cnt > 0 ? 1.0f - sum / (float)cnt : 1.0f;
        int ds = lane;
        if (lane >= kScSectors) d = INFINITY;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float od = __shfl_xor(d, o, kWave);
            const int os = __shfl_xor(ds, o, kWave);
            if (od < d || (od == d && os < ds)) { d = od; ds = os; }
        }
        if (active && lane == 0) {
            a.dist[(int64_t)q * a.n_db + cand] = d;
            a.shift[(int64_t)q * a.n_db + cand] = ds;
        }
        __syncthreads();                             // G is read: the next candidate may overwrite it
    }
}

// ------------------------------------------------------------------------------ selection
constexpr int kScSelT = 256;

__global__ __launch_bounds__(kScSelT) void k_sc_select(const float* __restrict__ dist,
                                                       const int32_t* __restrict__ shift, int n_db,
                                                       const int32_t* __restrict__ n_eligible,
                                                       ssf_sc_best* __restrict__ best) {
    __shared__ float sd[kScSelT / 64];
    __shared__ int si[kScSelT / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q = blockIdx.x;
    int n = n_eligible[q];
    n = n < 0 ? 0 : (n > n_db ? n_db : n);           // the host checked its copy
    float bd = INFINITY;
    int bi = INT_MAX;
    for (int i = tid; i < n; i += kScSelT) {
        float d = dist[(int64_t)q * n_db + i];
        d = d == d ? d : INFINITY;
        if (d < bd || bi == INT_MAX) { bd = d; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float od = __shfl_xor(bd, o, kWave);
        const int oi = __shfl_xor(bi, o, kWave);
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    if (lane == 0) { sd[w] = bd; si[w] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kScSelT / 64; ++k)
            if (sd[k] < bd || (sd[k] == bd && si[k] < bi)) { bd = sd[k]; bi = si[k]; }
        ssf_sc_best o;
        o.reserved = 0;
        if (n == 0) {
            o.index = -1; o.dist = 1.0f; o.shift = 0;
        } else {
            o.index = bi; o.dist = dist[(int64_t)q * n_db + bi]; o.shift = shift[(int64_t)q * n_db + bi];
        }
        best[q] = o;
    }
}

// Greedy top-K with an exclusion window (include/ssf_frontend.h): k rounds of k_sc_select's
// reduction over the candidates whose index differs by more than `exclusion` from every index
// taken so far.  The taken indices sit in LDS (copied to registers at the start of a round); every
// thread reads the round's winner from the four wave slots, so the round count and the early end
// are uniform.  The row is read again in every round.  Round 0 has nothing taken and is
// k_sc_select's reduction, comparison for comparison: slot 0 is its `best`.
constexpr int kScMaxTopk = SSF_SC_MAX_TOPK;

__global__ __launch_bounds__(kScSelT) void k_sc_select_topk(const float* __restrict__ dist,
                                                            const int32_t* __restrict__ shift, int n_db,
                                                            const int32_t* __restrict__ n_eligible, int k,
                                                            int exclusion, ssf_sc_best* __restrict__ best) {
    __shared__ float sd[kScSelT / 64];
    __shared__ int si[kScSelT / 64];
    __shared__ int taken[kScMaxTopk];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q = blockIdx.x;
    int n = n_eligible[q];
    n = n < 0 ? 0 : (n > n_db ? n_db : n);           // the host checked its copy
    const float* drow = dist + (int64_t)q * n_db;
    const int32_t* srow = shift + (int64_t)q * n_db;
    ssf_sc_best* out = best + (int64_t)q * k;
    int n_taken = 0;
    for (; n_taken < k; ++n_taken) {
        float bd = INFINITY;
        int bi = INT_MAX;
        int tk[kScMaxTopk];                              // the taken indices in registers for this round
#pragma unroll
        for (int j = 0; j < kScMaxTopk; ++j) tk[j] = j < n_taken ? taken[j] : 0;
        // the load does not wait for the window test, so the unrolled loads are in flight together
#pragma unroll 4
        for (int i = tid; i < n; i += kScSelT) {
            float d = drow[i];
            bool free = true;
#pragma unroll
            for (int j = 0; j < kScMaxTopk; ++j) {
                const int gap = i - tk[j];               // both in [0, n_db): no overflow
                free = free && (j >= n_taken || (gap < 0 ? -gap : gap) > exclusion);
            }
            d = d == d ? d : INFINITY;
            if (free && (d < bd || bi == INT_MAX)) { bd = d; bi = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float od = __shfl_xor(bd, o, kWave);
            const int oi = __shfl_xor(bi, o, kWave);
            if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
        }
        if (lane == 0) { sd[w] = bd; si[w] = bi; }
        __syncthreads();
        bd = sd[0]; bi = si[0];
        for (int m = 1; m < kScSelT / 64; ++m)
            if (sd[m] < bd || (sd[m] == bd && si[m] < bi)) { bd = sd[m]; bi = si[m]; }
        if (bi == INT_MAX) break;                        // the prefix is exhausted, for every thread
        if (tid == 0) taken[n_taken] = bi;
        __syncthreads();                                 // `taken` is written, the wave slots are read
    }
    // thread j writes slot j after the last round, so no round waits for a record's loads; a slot
    // that found no candidate gets the record k_sc_select writes without one
    if (tid < k) {
        ssf_sc_best o;
        o.index = -1; o.dist = 1.0f; o.shift = 0; o.reserved = 0;
        if (tid < n_taken) {
            const int i = taken[tid];
            o.index = i; o.dist = drow[i]; o.shift = srow[i];
        }
        out[tid] = o;
    }
}

// The dist / shift rows of every query against candidates 0 .. n_cols - 1 (n_cols > 0).
static hipError_t launch_sc_rows(hipStream_t s, int n_query, const float* query, int n_db, int n_cols,
                                 const float* db, float* dist, int32_t* shift) {
    static hipError_t once = hipFuncSetAttribute((const void*)k_sc_match,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kScMatchLds);
    if (once != hipSuccess) return once;
    ScMatchArgs a;
    a.query = query; a.db = db; a.dist = dist; a.shift = shift; a.n_db = n_db; a.n_cols = n_cols;
    a.groups = (n_cols + kScMatchW * kScCpw - 1) / (kScMatchW * kScCpw);
    kmark(s, "k_sc_match");
    hipLaunchKernelGGL(k_sc_match, dim3((unsigned)((int64_t)n_query * a.groups)), dim3(kScMatchT), kScMatchLds,
                       s, a);
    return hipGetLastError();
}

hipError_t launch_sc_match(hipStream_t s, int n_query, const float* query, int n_db, int n_cols, const float* db,
                           const int32_t* n_eligible, float* dist, int32_t* shift, ssf_sc_best* best) {
    if (n_query <= 0) return hipSuccess;
    if (n_cols > 0) {
        hipError_t e = launch_sc_rows(s, n_query, query, n_db, n_cols, db, dist, shift);
        if (e != hipSuccess) return e;
    }
    kmark(s, "k_sc_select");
    hipLaunchKernelGGL(k_sc_select, dim3(n_query), dim3(kScSelT), 0, s, dist, shift, n_db, n_eligible, best);
    return hipGetLastError();
}

hipError_t launch_sc_match_topk(hipStream_t s, int n_query, const float* query, int n_db, int n_cols,
                                const float* db, const int32_t* n_eligible, float* dist, int32_t* shift, int k,
                                int exclusion, ssf_sc_best* best) {
    if (k < 1 || k > kScMaxTopk) return hipErrorInvalidValue;   // `taken` holds kScMaxTopk indices
    if (n_query <= 0) return hipSuccess;
    if (n_cols > 0) {
        hipError_t e = launch_sc_rows(s, n_query, query, n_db, n_cols, db, dist, shift);
        if (e != hipSuccess) return e;
    }
    kmark(s, "k_sc_select_topk");
    hipLaunchKernelGGL(k_sc_select_topk, dim3(n_query), dim3(kScSelT), 0, s, dist, shift, n_db, n_eligible, k,
                       exclusion, best);
    return hipGetLastError();
}

}  // namespace ssf
