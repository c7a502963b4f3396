// mask_common.hpp -- what every stage of k_mask_pose (mask_pose.hip) shares: the tuning
// constants, the work-group's LDS state (MaskShared), the point loads and the streaming loops.
#pragma once
#include "ssf_device.hpp"
#include "ssf_internal.hpp"

#include <float.h>
#include <type_traits>

namespace ssf {

#ifndef SSF_MASK_THREADS
#define SSF_MASK_THREADS 768
#endif
constexpr int kMaskThreads = SSF_MASK_THREADS;   // 12 waves: 3 per SIMD at <= 168 VGPRs

// Diagnostic build only (-DSSF_MASK_STAMPS, libssf_frontend_diag.so): lane 0 records the
// s_memtime cycle count at each phase boundary into the frame's unused out slots 26..31.
// The product library is compiled without it; no product output is computed from a stamp.
#ifdef SSF_MASK_STAMPS
#define SSF_STAMP(slot)                                                                   \
    do {                                                                                  \
        if (threadIdx.x == 0) {                                                           \
            const unsigned long long _t = __builtin_amdgcn_s_memtime();                   \
            out[26 + (slot)] = (double)(_t - stamp0);                                     \
        }                                                                                 \
    } while (0)
#else
#define SSF_STAMP(slot) do { } while (0)
#endif
constexpr int kNW = kMaskThreads / 64;
#ifndef SSF_LLOYD_DEEP
#define SSF_LLOYD_DEEP 2
#endif
constexpr int kLloydDeep = SSF_LLOYD_DEEP;   // points in flight per thread in the Lloyd passes
#ifndef SSF_KPP_DEEP
#define SSF_KPP_DEEP 2
#endif
constexpr int kKppBlocks = 4096;             // k-means++ block totals in LDS (frames up to ~262k points)
constexpr double kPi = 3.14159265358979323846;
#ifndef SSF_LLOYD_FULL_PASSES
#define SSF_LLOYD_FULL_PASSES 4
#endif
constexpr int kLloydFullPasses = SSF_LLOYD_FULL_PASSES;   // full Lloyd passes before skipping
#ifndef SSF_LLOYD_REFULL
#define SSF_LLOYD_REFULL 4
#endif
constexpr int kLloydRefull = SSF_LLOYD_REFULL;   // back to a full pass when > n / this relabel
#ifndef SSF_LLOYD_REC_DEEP
#define SSF_LLOYD_REC_DEEP 8
#endif
constexpr int kLloydRecDeep = SSF_LLOYD_REC_DEEP;         // 16-byte record loads in flight per lane
constexpr int kLQ = SSF_LLOYD_REC_DEEP * 128;   // a record trip: D loads of two records per lane
constexpr int kLloydMax = 300;               // sklearn KMeans max_iter (pass index fits 9 bits)

// packed upper-triangular index of a 6x6 matrix (row i <= col j)
SSF_DEV constexpr int up(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }

// Everything lane 0 touches between passes lives here, in LDS: no private arrays, so the
// streaming passes keep the whole VGPR budget (1024 threads -> <= 128 VGPRs per lane).
struct MaskShared {
    double mean[6], tol;
    double tot[28];            // {N, sum(x-mean)[6], sum(x-mean)(x-mean)^T [21 packed]}
    double cen[12], csn[2], cenp[12], csnp[2];   // current / previous Lloyd centres
    double x0[6], ktot[16];    // pass-0 shift (point 0) and total Kabsch sums about it
    double logdet[2], logw[2];
    double Aq[21], bq[6], cq, C0;  // EM difference form: delta = a1 - a0 = v'A v + b'v + c (v = x - mean)
    double lb;
    double C[36], L[36];       // gmm_params2: the two components' precision matrices P0, P1
    double sums[29];           // lane 0's copy of a pass's block sums (never a per-lane array)
    double lsum[14];           // running Lloyd cluster sums {n0, S0[6], n1, S1[6]} about mean
    double lhist[kLloydMax * 9];   // per labelling pass t: w = c1 - c0 [6], s = csn0 - csn1,
                                   // |c0| + |c1|, csn0 + csn1 (lloyd_skip_bounds)
    float lb1[512], lb2[512];   // this pass's drift bounds against pass r (9-bit index)
    int64_t c0, c1;
    double dg_cyc, dg_n, dg_lab, dg_wfull, dg_full1;   // diagnostic build only
#ifdef SSF_MASK_STAMPS
    double dg_e[3];            // EM pass: points + block sum, exchange, M-step (cycles, summed)
#endif
    double passes;             // algorithmic bytes / (24 B x n): 1 per full pass (see the Lloyd loop)
    int km_iter, em_iter, strict, converged, done, status, label0, bg, bg_pred, lfull;
    double hnk[2], hq[2], hpm[12];   // gmm_params2: per-component results of lanes 0 / 1
    int hrc[2];
};

// T: the storage type of pos / flow (float: LiDAR data; double: the f64 Python boundary).
template <class T>
SSF_DEV void load_x(const T* __restrict__ P, const T* __restrict__ Fl, int64_t i, double x[6]) {
    x[0] = (double)Fl[3 * i]; x[1] = (double)Fl[3 * i + 1]; x[2] = (double)Fl[3 * i + 2];
    x[3] = (double)P[3 * i];  x[4] = (double)P[3 * i + 1];  x[5] = (double)P[3 * i + 2];
}

typedef __attribute__((address_space(3))) const double LdsDouble;

// The LDS address of the E-step parameters laundered through a VGPR once per point: the compiler can neither
// hoist the 27 loop-invariant doubles into VGPRs nor has to rebuild each address in an SGPR
// (one VGPR base, immediate ds_read2 offsets).  The low 32 bits of a generic LDS pointer are
// its LDS offset.
SSF_DEV const LdsDouble* lds_laundered(const double* p) {
    uint32_t a = (uint32_t)(uintptr_t)p;
    asm volatile("" : "+v"(a));
    return (const LdsDouble*)(uintptr_t)a;
}

// The streaming loops keep a thread's NEXT points' loads in flight as the raw six values,
// converted when used, while it computes the current one.
template <class T>
SSF_DEV void load_raw(const T* __restrict__ P, const T* __restrict__ Fl, int64_t i, T r[6]) {
    r[0] = Fl[3 * i]; r[1] = Fl[3 * i + 1]; r[2] = Fl[3 * i + 2];
    r[3] = P[3 * i];  r[4] = P[3 * i + 1];  r[5] = P[3 * i + 2];
}

// Cache policy of the point streams.  A frame's [flow, xyz] is 2.88 MB and
// hundreds of frames are in flight, so no point byte read by a loop over a whole part is found
// in a cache again: those loops (for_points_deep, for_point_pairs, the k-means++ distance stream
// of a part above kKppBlocks blocks)
// read with the non-temporal policy, global_load ... nt, and leave the L2 to the bytes that are
// re-used -- the Lloyd records, the relabel queues and the gathers of relabelled points, which
// stay at the default policy like every single-point read (each measured with nt and slower or
// equal).  SSF_NT_POINTS=0 builds the default-policy loads for an A/B.
#ifndef SSF_NT_POINTS
#define SSF_NT_POINTS 1
#endif
#if SSF_NT_POINTS
#define SSF_STREAM_LOAD(p) __builtin_nontemporal_load(p)
#else
#define SSF_STREAM_LOAD(p) (*(p))
#endif

// load_raw for a loop that streams a whole part
template <class T>
SSF_DEV void load_raw_stream(const T* __restrict__ P, const T* __restrict__ Fl, int64_t i, T r[6]) {
    r[0] = SSF_STREAM_LOAD(&Fl[3 * i]); r[1] = SSF_STREAM_LOAD(&Fl[3 * i + 1]); r[2] = SSF_STREAM_LOAD(&Fl[3 * i + 2]);
    r[3] = SSF_STREAM_LOAD(&P[3 * i]);  r[4] = SSF_STREAM_LOAD(&P[3 * i + 1]);  r[5] = SSF_STREAM_LOAD(&P[3 * i + 2]);
}

// three consecutive Ts at byte offset o (< 2^32) of a wave-uniform base: the global_load's SGPR
// base + 32-bit VGPR offset form, so the clamped index costs a min and a multiply per point
// instead of 64-bit compares, selects and address arithmetic.  Only the whole-part streams use
// it, so it reads with their policy (one global_load_dwordx3 ... nt for float).
template <class Ts>
SSF_DEV void load3_off(const Ts* __restrict__ base, uint32_t o, Ts r[3]) {
    const Ts* p = reinterpret_cast<const Ts*>(reinterpret_cast<const char*>(base) + o);
    r[0] = SSF_STREAM_LOAD(&p[0]); r[1] = SSF_STREAM_LOAD(&p[1]); r[2] = SSF_STREAM_LOAD(&p[2]);
}

// A wave-uniform LDS value moved to SGPRs: the per-point loops keep their VGPRs for the point
// data and the accumulators (1024-thread work-groups leave 128 VGPRs per lane).
SSF_DEV double uni(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                            __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// Points [r0, r1) of the frame (the work-group's part, see Split) streamed through fn, D points
// in flight per thread (a rolling register buffer of raw floats): thread t visits r0 + t,
// r0 + t + T, ... in order, whatever D, so every sum is bit-identical across depths.
// fn(i, x, val) runs for every slot of the last trip too (val = false past r1, x = the clamped
// last point): a store under a branch in a streaming loop made the compiler drain the prefetches
// at the join (the record-writing full pass took 411 k cycles against 264 k without records).
// kWaveTrips: a wave makes its trips together -- a lane whose own points have run out goes on
// with val = false slots while any lane of its wave has one, so fn may use cross-lane operations
// over whole 64-point blocks (wave w holds block (j >> 6) of the part at slot j).  The extra
// slots add zeros: the sums keep their bits.
template <int D, bool kWaveTrips = false, class Ts, class Fn>
SSF_DEV void for_points_deep(const Ts* __restrict__ P, const Ts* __restrict__ Fl, int64_t r0, int64_t r1, Fn&& fn) {
    // frames of at most 2^32 / (3 sizeof(Ts)) points (mask_pose_batch rejects larger ones)
    if (r1 <= r0) return;                              // uniform (an empty part)
    const Ts* Pb = P + 3 * r0;
    const Ts* Fb = Fl + 3 * r0;
    const uint32_t n = (uint32_t)(r1 - r0), T = blockDim.x, last = n - 1;
    constexpr uint32_t S = 3 * sizeof(Ts);
    const uint32_t j0 = threadIdx.x;
    const uint32_t lead = kWaveTrips ? (j0 & 63u) : 0u;   // the lane's offset in its 64-point block
    auto load = [&](uint32_t k, Ts r[6]) { load3_off(Fb, k * S, r); load3_off(Pb, k * S, r + 3); };
    Ts buf[D][6];
#pragma unroll
    for (int d = 0; d < D; ++d) load(min(j0 + d * T, last), buf[d]);
    for (uint32_t base = j0; base - lead < n; base += D * T) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const uint32_t j = base + d * T;
            double x[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) x[k] = (double)buf[d][k];
            load(min(j + D * T, last), buf[d]);
            fn(r0 + (int64_t)j, x, j < n);
        }
    }
}

// EM: two points per step (i, i + T) so every parameter read serves both: fn2(xa, xb) for every
// full pair, then fn1(xa) for a thread's lone last point (its second point does not exist), so
// the pair body carries no weight for a missing point.  Loads clamped and unconditional (a
// counted wait); the next step's pair is held in registers.  Two register
// pairs in flight, or the loop unrolled with swapping register sets, were 6 % / 4 % slower (the
// compiler waits for the loads right after issuing them, r6t / r6u); DESIGN 6.1 lists the other
// forms that were measured and not kept.
template <class Ts, class Fn2, class Fn1>
SSF_DEV void for_point_pairs(const Ts* __restrict__ P, const Ts* __restrict__ Fl, int64_t r0, int64_t r1, Fn2&& fn2,
                             Fn1&& fn1) {
    // frames of at most 2^32 / (3 sizeof(Ts)) points (mask_pose_batch rejects larger ones)
    const Ts* Pb = P + 3 * r0;
    const Ts* Fb = Fl + 3 * r0;
    const uint32_t n = (uint32_t)(r1 - r0), T = blockDim.x, last = n - 1;
    constexpr uint32_t S = 3 * sizeof(Ts);
    uint32_t i = threadIdx.x;
    if (i >= n) return;
    Ts ra[6], rb[6];
    auto load = [&](uint32_t k, Ts r[6]) { load3_off(Fb, k * S, r); load3_off(Pb, k * S, r + 3); };
    load(i, ra);
    load(min(i + T, last), rb);
    for (; i + T < n; i += 2 * T) {
        double xa[6], xb[6];
#pragma unroll
        for (int d = 0; d < 6; ++d) { xa[d] = (double)ra[d]; xb[d] = (double)rb[d]; }
        load(min(i + 2 * T, last), ra);
        load(min(i + 3 * T, last), rb);
        fn2(xa, xb);
    }
    if (i < n) {                                       // ra holds point i
        double xa[6];
#pragma unroll
        for (int d = 0; d < 6; ++d) xa[d] = (double)ra[d];
        fn1(xa);
    }
}

}  // namespace ssf
