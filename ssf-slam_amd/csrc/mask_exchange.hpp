// mask_exchange.hpp -- one frame of k_mask_pose over G work-groups: the Split, the exchange of
// block totals between a frame's parts, and what a stage is handed (MaskCtx, MaskLds).
#pragma once
#include "mask_common.hpp"

namespace ssf {

// ---- one frame over G work-groups --------------------------------------------------------
// With G > 1 (small batches: G x frames fills the chip; see launch_mask_pose) every frame is
// cut into G contiguous parts of its points, one work-group each.  Each pass then sums over
// the work-group's part and the G partial sums are exchanged through global memory: every part
// stores its block totals write-through (sc1, relaxed agent-scope atomic stores) into its slot,
// drains them (s_waitcnt vmcnt(0)) and adds 1 to the frame's arrival counter; lane 0 polls the
// counter (relaxed agent loads, s_sleep) until all G parts of this exchange have arrived, and
// the totals are read back with sc1 loads and added in part order -- so every work-group of the
// frame holds the same bits and runs the same lane-0 algebra to the same decisions
// (cdna_hip_programming.md Guideline 16, MI355X_MICROARCH.md "Valid forms", row 1: one
// storing wave, one atomic-add signal, sc1 polls and sc1 loads, one work-group per CU).
// Every exchange of a launch has its OWN slot lines (slot = exchange index), never a line
// rewritten in the launch: an sc1 load bypasses the CU's L1 but is served by the reader XCD's
// L2 when that L2 already holds the line, and another XCD's sc1 store does not reach that copy.
// Measured on MI355X with a work-sharing variant of this kernel that re-read rewritten
// parameter lines across XCDs: 375-810 stale reads per 256-frame launch.  A
// line read here for the first time cannot be cached stale.
// Work-groups take (frame, part) tickets in order from a counter, so every partly started frame
// has its parts on resident work-groups and the ones it waits for are taken by the next
// work-group that becomes free (no wait on a work-group that cannot be dispatched).  A bounded
// spin turns a lost partner into status SSF_POSE_SYNC_FAILED, never a hang.
constexpr int kSlot = 32;                         // doubles per part and exchange
constexpr int kMaxSplit = kMaskMaxSplit;          // parts per frame at most (32)
constexpr uint32_t kSpinLimit = 1u << 24;         // x s_sleep 2 (~128 cycles): ~1 s
// exchanges per frame at most: pass 0, 3 in k-means++, one per Lloyd iteration (<= 300), the
// GMM init, one per EM iteration (<= 100), the final pass
constexpr int kMaxExchanges = 1 + 3 + 300 + 1 + 100 + 1;

struct Split {
    int G, g;                  // parts per frame, this work-group's part
    int64_t r0, r1;            // its points [r0, r1) of the frame
    double* part;              // the frame's slots [kMaxExchanges][G][kSlot]
    uint32_t* arrive;          // the frame's arrival counter (monotonic over its exchanges)
    uint32_t* fail;            // the frame's failure word: set by any part whose wait timed out
    uint32_t seq;              // exchanges done (uniform)
};

// What every stage of the fit is handed: the frame part it works on ...
template <class T>
struct MaskCtx {
    const T* P;                // the frame's points and flow (point 0 of the frame at index 0)
    const T* Fl;
    int64_t fb, n;             // the frame's first point in the batch, its point count
    int f;                     // the frame
    double* out;               // its SSF_POSE_OUT_STRIDE output doubles
    Split X;
    double mean[6];            // column means in SGPRs, once pass 0 has produced them
};

// ... and the kernel's LDS arrays (declared in k_mask_pose).
struct MaskLds {
    MaskShared& S;
    double (&red)[kNW * 32];
    int (&ired)[kNW];
    unsigned long long (&cand)[2];
    double (&bsum)[kKppBlocks];                   // k-means++ per-64-point-block distance totals
    uint32_t (&lq)[kNW * kLQ];                    // Lloyd skip passes: per-wave relabel entries of a trip
    double (&xtmp)[kSlot + kMaxSplit * kSlot];    // exchange totals + the gathered parts
    int& okflag;
};

// The write-through form below matches a measured valid hand-off (MI355X_MICROARCH.md "Valid
// forms", row 1), which the guide marks as measured on gfx950 / ROCm 7.2, not an architectural
// guarantee.  So the exchange also carries the architectural pair: an agent-scope release fence
// before the arrival add and an agent-scope acquire after the poll (round 3).  Cost,
// same box A/B: configs[1] latency 0.554 -> 0.574 ms, configs[2] as written 4868 -> 4715
// frames/s (tools/gpu/r3i.sh); B = 256 runs G = 1 and never exchanges.

// lane 0: wait until the frame's arrival counter reaches `target` (relaxed sc1 polls with
// s_sleep back-off); false when a partner reported a timeout or the spin bound ran out
SSF_DEV bool wait_arrivals(const Split& X, uint32_t target) {
    uint32_t spins = 0;
    while (__hip_atomic_load(X.arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(2);
        if (++spins > kSpinLimit ||
            __hip_atomic_load(X.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)
            return false;
    }
    return true;
}

// The signal and the wait of exchange number X.seq (already counted): wave 0, which stored every
// value, drains its stores; lane 0 adds the part's arrival and, when `wait`, polls until all G
// parts of this exchange have arrived.  *okflag (lane 0 writes it; read it after a barrier): 0
// when the wait failed.
SSF_DEV void signal_and_wait(const Split& X, int* okflag, bool wait = true) {
    if (threadIdx.x < 64) {                        // wave 0 stored every value
        // drain the write-through stores before the signal (R1); the asm is also the compiler
        // barrier that keeps them above the add
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_fetch_add(X.arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int ok = !wait || wait_arrivals(X, (uint32_t)X.G * X.seq) ? 1 : 0;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            *okflag = ok;
        }
    }
}

template <int N, bool kMin = false>
SSF_DEV bool exchange(Split& X, double (&v)[N], double* tmp, int* okflag) {
    static_assert(N <= kSlot, "exchange: N <= kSlot");
    if (X.G == 1) return true;
    if (X.seq >= (uint32_t)kMaxExchanges) return false;   // cannot happen (iteration caps); never reuse a line
    double* slot = X.part + (size_t)X.seq * (size_t)X.G * kSlot;
#pragma unroll
    for (int k = 0; k < N; ++k)
        if (threadIdx.x == (unsigned)k)
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(slot + X.g * kSlot + k),
                               (unsigned long long)__double_as_longlong(v[k]), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    X.seq += 1u;
    signal_and_wait(X, okflag);
    __syncthreads();
    // no instruction: keeps the compiler from moving the slot loads above the poll and the
    // barrier (the sc1 loads themselves stand in for the acquire: Guideline 16, Valid forms row 1)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (!*okflag) return false;                    // uniform
    // every (part, value) on its own thread: one load latency for the G x N values (a loop over
    // the parts per value waited for G loads in a row); tmp holds kMaxSplit x kSlot doubles
    for (int t = threadIdx.x; t < X.G * N; t += blockDim.x) {
        const int gg = t / N, k = t - gg * N;
        tmp[kSlot + t] = __longlong_as_double((long long)__hip_atomic_load(
            reinterpret_cast<unsigned long long*>(slot + gg * kSlot + k), __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_AGENT));
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)N) {
        double acc = kMin ? __builtin_inf() : 0.0;
        for (int gg = 0; gg < X.G; ++gg) {                 // part order: the same bits everywhere
            const double x = tmp[kSlot + gg * N + threadIdx.x];
            acc = kMin ? (x < acc ? x : acc) : acc + x;
        }
        tmp[threadIdx.x] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = tmp[k];
    __syncthreads();
    return true;
}

// One value per part; every part reads the G values in part order -> the sum over the parts
// before this one and the total (the k-means++ cumulative potential).  Same protocol as exchange.
SSF_DEV bool exchange_prefix(Split& X, double v, double* tmp, int* okflag, double& before, double& total) {
    if (X.seq >= (uint32_t)kMaxExchanges) return false;
    double* slot = X.part + (size_t)X.seq * (size_t)X.G * kSlot;
    if (threadIdx.x == 0)
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(slot + X.g * kSlot),
                           (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    X.seq += 1u;
    signal_and_wait(X, okflag);
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (!*okflag) return false;                    // uniform
    if (threadIdx.x < (unsigned)X.G)
        tmp[kSlot + threadIdx.x] = __longlong_as_double((long long)__hip_atomic_load(
            reinterpret_cast<unsigned long long*>(slot + threadIdx.x * kSlot), __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_AGENT));
    __syncthreads();
    if (threadIdx.x == 0) {
        double b = 0.0, t = 0.0;
        for (int gg = 0; gg < X.G; ++gg) {
            const double x = tmp[kSlot + gg];
            if (gg < X.g) b += x;
            t += x;
        }
        tmp[0] = b; tmp[1] = t;
    }
    __syncthreads();
    before = tmp[0];
    total = tmp[1];
    __syncthreads();
    return true;
}

// The done round (G > 1), after a part's share of the mask is written: every part signals, part 0
// alone waits, so its success status stands only once every part has finished (a part whose wait
// timed out returned early and set the failure word).  False, in lane 0 of part 0 only, when a
// part never arrived.
SSF_DEV bool done_round(Split& X, int* okflag) {
    __syncthreads();
    X.seq += 1u;
    signal_and_wait(X, okflag, X.g == 0);
    return threadIdx.x != 0 || *okflag != 0;
}

}  // namespace ssf
