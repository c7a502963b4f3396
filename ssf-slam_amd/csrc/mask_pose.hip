// mask_pose.hip -- the dynamic-point mask + Kabsch pose block of
// scripts/PointCloudOdometry_noSeg.py:97-125 (and PointCloudOdometry.py:91-101) on gfx950.
//
// One work-group owns one frame and runs the WHOLE GaussianMixture(n_components=2).fit_predict
// on device (sklearn 1.7.2 semantics, f64 arithmetic on the f32 point / flow storage):
//   pass 0      X = [flow, xyz]: column means and variances (KMeans centering, tol); the same
//               stream forms the distances to the first k-means++ centre (index chosen from the
//               caller's RandomState draw, so known before any point is read) and leaves their
//               totals per 64-point block
//   k-means++   in-order prefix scan over the block totals -> the two local-trial candidates;
//               one stream for their potentials, which also labels Lloyd iteration 0 against
//               (first centre, candidate) for both candidates: the winner's cluster sums are
//               that iteration's
//   Lloyd       from iteration 1: one streaming pass per iteration (labels, per-cluster sums,
//               changed-label count)
//   GMM init    one-hot responsibilities -> shifted first/second moments -> 6x6 Cholesky
//   EM          ONE fused pass per iteration: E-step (log-prob difference of the two components,
//               responsibilities) and the M-step moment sums of the next parameters together
//   final       argmax labels + per-label Kabsch sums (src = pos + flow, dst = pos) in one pass,
//               background = majority label, 3x3 SVD (one-sided Jacobi, f64) on one lane,
//               R, t, pyquaternion trace-method q; then one pass writes the uint8 mask.
// The small dense algebra runs between passes: the two components' Cholesky / difference form on
// lanes 0 and 1 in registers (gmm_params2), the SVD and convergence tests on lane 0;
// no host round trip for the whole fit.  Every pass is a coalesced stream of 24 B/point.
//
// This file holds the kernel -- the ticket loop, a frame part's context and the list of stage
// calls -- and the launchers.  Each stage is one forced-inline function template on the storage
// type, handed the frame part (MaskCtx) and the kernel's LDS arrays (MaskLds); it returns false
// when an exchange between the frame's parts failed.  The stages pass their results on in
// MaskShared (each stage's comment says what it reads and writes there):
//   mask_common.hpp    constants, MaskShared, the point loads and the streaming loops
//   mask_exchange.hpp  Split, the exchange between a frame's parts, MaskCtx, MaskLds
//   mask_seed.hpp      mask_pass0, mask_kmeanspp (ends in Lloyd iteration 0)
//   mask_lloyd.hpp     mask_lloyd, the lane-0 algebra around a labelling pass, and the layout of
//                      the record / queue buffer
//   mask_em.hpp        mask_gmm_init, mask_em
//   mask_final.hpp     mask_final, mask_flip, mask_given
//   mask_gmm.hpp       gmm_params2 and the per-point E-step pieces
//   mask_kabsch.hpp    accum_kabsch, kabsch_finish
#include "mask_seed.hpp"
#include "mask_lloyd.hpp"
#include "mask_em.hpp"
#include "mask_final.hpp"

namespace ssf {

template <class T>
__global__ __launch_bounds__(kMaskThreads) void k_mask_pose(
    const T* __restrict__ pts, const T* __restrict__ flow,
    const int64_t* __restrict__ frame_off, int mode, const uint8_t* __restrict__ mask_in,
    const double* __restrict__ draws, uint2* __restrict__ lloyd_rec, int reflection,
    uint8_t* __restrict__ bg_mask, double* __restrict__ out_all, int n_frames, int G,
    uint32_t* __restrict__ sync, double* __restrict__ parts, const int32_t* __restrict__ order,
    int tickets) {
    __shared__ MaskShared S;
    __shared__ double red[kNW * 32];
    __shared__ int ired[kNW];
    __shared__ unsigned long long cand_lds[2];
    __shared__ double bsum[kKppBlocks];   // k-means++ per-64-point-block distance totals
    __shared__ uint32_t lq[kNW * kLQ];     // Lloyd skip passes: per-wave relabel entries of a trip
    __shared__ double xtmp[kSlot + kMaxSplit * kSlot];   // exchange totals + the gathered parts
    __shared__ int tk, okflag;
    const MaskLds L{S, red, ired, cand_lds, bsum, lq, xtmp, okflag};
    const int tid = threadIdx.x;
    // G == 1 without tickets: work-group = frame.  Otherwise (frame, part) tickets in order (see
    // Split; with G == 1 a frame queue: a work-group takes the next frame when its frame is
    // done, so a slow frame holds one CU while the others drain the batch).  order (optional): the
    // k-th frame dispatched is order[k] (a permutation; results do not depend on it).
    for (int iter = 0;; ++iter) {
    int f, g = 0;
    if (G == 1 && !tickets) {
        if (iter > 0) break;
        f = blockIdx.x;
    } else {
        __syncthreads();                       // the previous frame's readers of S / tk are done
        if (tid == 0) tk = (int)atomicAdd(sync, 1u);
        __syncthreads();
        f = tk / G;
        g = tk - f * G;
        if (f >= n_frames) break;              // uniform: every wave leaves
    }
    if (order) {
        f = order[f];
        if ((unsigned)f >= (unsigned)n_frames) continue;   // uniform: not a frame (skipped)
    }
    [&]() {                                    // one frame part; `return` ends it
    const int64_t fb = frame_off[f], n = frame_off[f + 1] - fb;
    double* out = out_all + (int64_t)f * SSF_POSE_OUT_STRIDE;
    MaskCtx<T> C;
    C.P = pts + 3 * fb;
    C.Fl = flow + 3 * fb;
    C.fb = fb; C.n = n; C.f = f; C.out = out;
    Split& X = C.X;
    X.G = G; X.g = g;
    {
        const int64_t chunk = ((n + G - 1) / G + 127) / 128 * 128;   // parts start at even records
        X.r0 = min(n, (int64_t)g * chunk);
        X.r1 = min(n, X.r0 + chunk);
    }
    X.part = parts + (size_t)f * kMaxExchanges * (size_t)G * kSlot;
    X.arrive = sync + 4 + f;
    X.fail = sync + 4 + n_frames + f;
    X.seq = 0;
    auto sync_failed = [&]() {                 // a partner never arrived: report, never hang
        if (tid == 0) {
            // every part reports, so part 0 never publishes a frame whose other parts stopped
            // before their share of the mask (the done round below)
            __hip_atomic_store(X.fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (g == 0) {
                for (int i = 0; i < SSF_POSE_OUT_STRIDE; ++i) out[i] = 0.0;
                out[SSF_POSE_OUT_STATUS] = SSF_POSE_SYNC_FAILED;
            }
        }
    };
    // the M-step of mask_gmm_init / mask_em, called here so that gmm_params2 is handed S by name
    auto mstep = [&](int init) { return gmm_params2(S, S.sums, init, n); };
    if (tid == 0) {
        S.passes = 0; S.status = 0; S.km_iter = 0; S.em_iter = 0; S.converged = 0;
        if (g == 0) for (int i = 26; i < SSF_POSE_OUT_STRIDE; ++i) out[i] = 0.0;
    }
#ifdef SSF_MASK_STAMPS
    const unsigned long long stamp0 = __builtin_amdgcn_s_memtime();
#endif
    __syncthreads();

    if (mode != SSF_MASK_GMM) {
        mask_given(C, L, mode, mask_in, reflection, bg_mask);
        return;
    }
    if (n < 2) {
        if (tid == 0 && g == 0) {
            for (int i = 0; i < SSF_POSE_OUT_STRIDE; ++i) out[i] = 0.0;
            out[SSF_POSE_OUT_STATUS] = SSF_POSE_GMM_FAILED;
        }
        return;
    }

    if (!mask_pass0(C, L, draws)) { sync_failed(); return; }
    SSF_STAMP(0);
#pragma unroll
    for (int d = 0; d < 6; ++d) C.mean[d] = uni(S.mean[d]);
    if (!mask_kmeanspp(C, L, draws)) { sync_failed(); return; }
    SSF_STAMP(1);
    if (!mask_lloyd(C, L, lloyd_rec, frame_off[n_frames], n_frames)) { sync_failed(); return; }
    SSF_STAMP(2);
    if (!mask_gmm_init(C, L, mstep)) { sync_failed(); return; }
    SSF_STAMP(3);
    if (!mask_em(C, L, mstep)) { sync_failed(); return; }
    SSF_STAMP(4);
    if (!mask_final(C, L, reflection, bg_mask)) { sync_failed(); return; }
    mask_flip(C, L, bg_mask);
    if (G > 1 && !done_round(X, &okflag)) {    // false in lane 0 of part 0 only
        for (int i = 0; i < SSF_POSE_OUT_STRIDE; ++i) out[i] = 0.0;
        out[SSF_POSE_OUT_STATUS] = SSF_POSE_SYNC_FAILED;
    }
    SSF_STAMP(5);
    }();                                       // the frame part
    }                                          // tickets
}

template <class T>
hipError_t launch_mask_pose(hipStream_t s, int n_frames, const MaskPlan& plan, const MaskArgs<T>& a) {
    if (n_frames <= 0) return hipSuccess;
    if (plan.tickets) {
        // zero the ticket and arrival counters (16-byte multiple, from the allocation start)
        const size_t zb = (mask_sync_bytes(n_frames) + 15) & ~(size_t)15;
        hipError_t e = hipMemsetAsync(a.sync, 0, zb, s);
        if (e != hipSuccess) return e;
    }
    kmark(s, sizeof(T) == 8 ? "k_mask_pose_f64" : "k_mask_pose");
    hipLaunchKernelGGL(k_mask_pose<T>, dim3(plan.grid), dim3(kMaskThreads), 0, s, a.pts, a.flow, a.frame_off,
                       a.mode, a.mask_in, a.draws, a.lloyd_rec, a.reflection, a.bg_mask, a.out, n_frames, plan.G,
                       a.sync, a.parts, a.order, plan.tickets ? 1 : 0);
    return hipGetLastError();
}

// One storage type per translation unit (mask_pose_f64.hip compiles this file again with
// SSF_MASK_F64_TU), so the float kernel's code generation does not depend on the f64 variant.
#ifndef SSF_MASK_F64_TU
template hipError_t launch_mask_pose<float>(hipStream_t, int, const MaskPlan&, const MaskArgs<float>&);

int mask_pose_slots(int device) {
    int cus = 0, per = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_mask_pose<float>, kMaskThreads, 0) != hipSuccess) return 0;
    return cus * per;
}

// ticket words, then per frame its arrival counter and its failure word
size_t mask_sync_bytes(int n_frames) { return (size_t)(4 + 2 * n_frames) * sizeof(uint32_t); }
size_t mask_parts_bytes(int n_frames, int G) {
    return G > 1 ? (size_t)n_frames * kMaxExchanges * G * kSlot * sizeof(double) : 0;
}
// the Lloyd records, then the relabel queues (mask_lloyd.hpp: lloyd_rec_base, lloyd_queue_base)
size_t mask_rec_bytes(int64_t total, int n_frames) {
    return sizeof(uint2) * (size_t)lloyd_rec_count(total, n_frames) +
           sizeof(uint32_t) * (size_t)lloyd_queue_count(total, n_frames);
}

MaskPlan mask_plan(int n_frames, int64_t total, int mode, int split, int slots, int queue) {
    MaskPlan p{};
    p.G = split > 0 ? split : slots > 0 ? slots / n_frames : 1;
    p.G = std::max(1, std::min(p.G, kMaxSplit));
    if (mode != SSF_MASK_GMM) p.G = 1;
    p.queue = p.G == 1 && queue > 0 && queue < n_frames ? queue : 0;
    p.tickets = p.G > 1 || p.queue > 0;
    const int64_t want = (int64_t)n_frames * p.G;       // with tickets: at most cap work-groups
    const int cap = p.G > 1 ? slots : p.queue;
    p.grid = (int)(p.tickets && cap > 0 && want > cap ? cap : want);
    p.draws_bytes = sizeof(double) * 3 * (size_t)n_frames;
    p.rec_bytes = mode == SSF_MASK_GMM ? mask_rec_bytes(total, n_frames) : 0;
    p.sync_bytes = p.tickets ? mask_sync_bytes(n_frames) + 16 : 0;
    p.parts_bytes = mask_parts_bytes(n_frames, p.G);
    return p;
}
#else
template hipError_t launch_mask_pose<double>(hipStream_t, int, const MaskPlan&, const MaskArgs<double>&);
#endif

}  // namespace ssf
