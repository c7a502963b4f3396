// subsample.hip -- the loader's point subsample (utils/datasets/carla.py:179-200, 236-250, 274-285:
// rm_ground cut, hybrid fg/bg quota, np.random.choice to nb_points) as one seeded, exactly
// specified device launch for all clouds of a step (ssf_subsample_batch), on gfx950.
//
// The reference draws from numpy's global MT19937 on the host, per frame.  Here the draw is a
// counter-based key per point:
//   F        the SplitMix64 finaliser;  g = 0x9E3779B97F4A7C15
//   s(st)    = F(F(F(seed + g) + tag) + st)                       st: 0 selection, 1 resampling
//   key(st, i) = (F(s(st) + (i + 1) g) >> 32) >> (32 - key_bits)   i: index within the frame
// without replacement (survivors n > nb): the nb survivors smallest in (key(0, i), i), ascending;
// with replacement (1 <= n <= nb): slot j takes the survivor of rank (key(1, j) * n) >> 32;
// quota: min(n_fg, quota) smallest-key foreground survivors, then the smallest-key background.
//
// One 1024-thread work-group per frame; nothing is exchanged between work-groups.  The order
// (key, i) is the order of the 64-bit composite c = key << (64 - key_bits) | i, which is unique
// per point, so "the m smallest" has no ties: a radix select over c's digits (12, 12, 8 bits of
// the key, then 12, 12 bits of the index; keys recomputed from the index on every pass, never
// stored; a 4096-bin LDS histogram per pass) ends as soon as the chosen bin holds exactly what is
// still needed -- after two passes for 32-bit keys on a 120 k cloud, the index passes run only
// when keys tie.  The last pass gathers the m <= 8192 composites into LDS (64 KiB, the histogram
// lives in the same bytes), a bitonic sort orders them, and the indices and the gathered xyz
// (channel-major) are written with plain vector stores.  Only LDS atomics are used.
#include "ssf_device.hpp"
#include "ssf_internal.hpp"

namespace ssf {

constexpr int kSubT = 1024;                         // threads per work-group
constexpr int kSubMax = SSF_SAMPLE_MAX_NB;          // composites the sort buffer holds
constexpr int kSubBins = 4096;                      // histogram bins: the widest digit is 12 bits
constexpr size_t kSubLds = (size_t)kSubMax * 8;     // dynamic LDS: the sort buffer / histogram

struct SubCtl {                // block-wide state of one frame (static LDS)
    uint32_t wsum[kSubT / 64];
    uint32_t n, n_fg;          // survivors, foreground survivors
    uint32_t bin, less, cnt;   // find_bin: the chosen bin, the count below it, the count in it
    uint32_t fill;             // gather cursor
};

SSF_DEV uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
constexpr uint64_t kGamma = 0x9E3779B97F4A7C15ull;

// the high word of the (i + 1)-th output of SplitMix64 seeded with s
SSF_DEV uint32_t key32(uint64_t s, uint32_t i) { return (uint32_t)(mix64(s + ((uint64_t)i + 1) * kGamma) >> 32); }

struct SubFrame {              // what a thread needs to classify point i of its frame
    const float* z;            // &pts[b * stride + 2], or null: no cut
    const uint8_t* cls;        // &cls[b], or null
    int stride;
    float z_min;
    uint64_t s0;               // s(0)
    uint32_t kmask;            // the key bits kept: high key_bits of the 32-bit word
};

enum { kAll = 0, kFg = 1, kBg = 2 };

SSF_DEV bool survives(const SubFrame& fr, uint32_t i) {
    return !fr.z || !(fr.z[(int64_t)i * fr.stride] < fr.z_min);
}

// point i belongs to the set `kind` draws from
SSF_DEV bool member(const SubFrame& fr, int kind, uint32_t i) {
    if (!survives(fr, i)) return false;
    if (kind == kAll) return true;
    const bool fg = fr.cls[i] != 0;
    return kind == kFg ? fg : !fg;
}

SSF_DEV uint64_t composite(const SubFrame& fr, bool keyed, uint32_t i) {
    return keyed ? ((uint64_t)(key32(fr.s0, i) & fr.kmask) << 32) | i : (uint64_t)i;
}

// The bin where the running count of hist[] reaches `rem` (1 <= rem <= the histogram's total):
// ctl.bin, ctl.less = the count below that bin, ctl.cnt = the count in it.
SSF_DEV void find_bin(const uint32_t* hist, uint32_t rem, SubCtl& ctl) {
    const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    uint32_t h[kSubBins / kSubT], s = 0;
#pragma unroll
    for (int k = 0; k < kSubBins / kSubT; ++k) { h[k] = hist[tid * (kSubBins / kSubT) + k]; s += h[k]; }
    uint32_t inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(inc, o, kWave);
        if (lane >= o) inc += v;
    }
    if (lane == 63) ctl.wsum[w] = inc;
    __syncthreads();
    uint32_t ex = inc - s;
    for (int k = 0; k < w; ++k) ex += ctl.wsum[k];
#pragma unroll
    for (int k = 0; k < kSubBins / kSubT; ++k) {
        if (ex < rem && rem <= ex + h[k]) {
            ctl.bin = (uint32_t)(tid * (kSubBins / kSubT) + k);
            ctl.less = ex;
            ctl.cnt = h[k];
        }
        ex += h[k];
    }
    __syncthreads();
}

// The m smallest composites of the set `kind` (1 <= m <= kSubMax, the set holds at least m), or
// with keyed = false the whole set by index (the set holds exactly m), sorted ascending into
// buf[0 .. m).  Every thread of the work-group calls it; buf is also the histogram.
SSF_DEV void select_sorted(const SubFrame& fr, int kind, bool keyed, uint32_t N, uint32_t m,
                           uint64_t* buf, SubCtl& ctl) {
    const int tid = threadIdx.x;
    uint32_t* hist = reinterpret_cast<uint32_t*>(buf);
    // ---- radix select: the threshold is "c >> sh <= pfx" -----------------------------------
    int sh = 0;
    uint64_t pfx = ~0ull;                       // keyed = false: every member
    if (keyed) {
        constexpr int kShift[5] = {52, 40, 32, 12, 0};
        constexpr int kBits[5] = {12, 12, 8, 12, 12};
        uint32_t rem = m;
        int prev = 64;
        pfx = 0;
        for (int p = 0; p < 5; ++p) {
            for (int k = tid; k < kSubBins; k += kSubT) hist[k] = 0;
            __syncthreads();
            sh = kShift[p];
            const uint32_t dmask = (1u << kBits[p]) - 1u;
            for (uint32_t i = tid; i < N; i += kSubT) {
                if (!member(fr, kind, i)) continue;
                const uint64_t c = composite(fr, true, i);
                if (p > 0 && (c >> prev) != pfx) continue;
                atomicAdd(&hist[(uint32_t)(c >> sh) & dmask], 1u);
            }
            __syncthreads();
            find_bin(hist, rem, ctl);
            pfx = (p > 0 ? pfx << (prev - sh) : 0ull) | ctl.bin;
            rem -= ctl.less;
            const bool done = rem == ctl.cnt;   // the whole bin is taken: no finer digit needed
            prev = sh;
            __syncthreads();                    // ctl is rewritten by the next pass
            if (done) break;
        }
    }
    // ---- gather (any order), pad to a power of two, bitonic sort ---------------------------
    if (tid == 0) ctl.fill = 0;
    __syncthreads();
    for (uint32_t i = tid; i < N; i += kSubT) {
        if (!member(fr, kind, i)) continue;
        const uint64_t c = composite(fr, keyed, i);
        if ((c >> sh) > pfx) continue;
        const uint32_t slot = atomicAdd(&ctl.fill, 1u);
        if (slot < (uint32_t)kSubMax) buf[slot] = c;
    }
    uint32_t P = 1;
    while (P < m) P <<= 1;
    __syncthreads();
    for (uint32_t k = m + tid; k < P; k += kSubT) buf[k] = ~0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < P / 2; t += kSubT) {
                const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const uint64_t a = buf[lo], b = buf[hi];
                if ((a > b) == ((lo & k) == 0)) { buf[lo] = b; buf[hi] = a; }
            }
            __syncthreads();
        }
    }
}

struct SubTags { uint64_t t[SSF_SAMPLE_TAG_CHUNK]; };

struct SubArgs {
    const float* pts;
    const int64_t* off;
    const uint8_t* cls;
    int32_t* idx;
    float* xyz;
    int32_t* n_out;
    int32_t* status;
    uint64_t seed;
    int stride, nb, use_z, quota, key_bits, frame0, use_tags;
    float z_min;
};

__global__ __launch_bounds__(kSubT) void k_subsample(SubArgs a, SubTags tags) {
    extern __shared__ uint64_t sub_buf[];
    __shared__ SubCtl ctl;
    const int tid = threadIdx.x;
    const int f = a.frame0 + (int)blockIdx.x;
    const int64_t b = a.off[f];
    const int64_t len = a.off[f + 1] - b;       // the host checked its copy against the limit
    const uint32_t N = len < 0 || len > (int64_t)SSF_SAMPLE_MAX_POINTS ? 0u : (uint32_t)len;
    const uint64_t tag = a.use_tags ? tags.t[blockIdx.x] : (uint64_t)f;
    const uint64_t sf = mix64(mix64(a.seed + kGamma) + tag);
    SubFrame fr;
    fr.stride = a.stride;
    fr.z = a.use_z ? a.pts + b * a.stride + 2 : nullptr;
    fr.cls = a.cls ? a.cls + b : nullptr;
    fr.z_min = a.z_min;
    fr.s0 = mix64(sf);
    fr.kmask = 0xFFFFFFFFu << (32 - a.key_bits);
    const uint64_t s1 = mix64(sf + 1);
    const bool quota = a.quota >= 0;
    int32_t* idx = a.idx + (int64_t)f * a.nb;
    float* xyz = a.xyz ? a.xyz + (int64_t)f * 3 * a.nb : nullptr;
    const float* pts = a.pts + b * a.stride;

    // ---- survivors and foreground survivors -------------------------------------------------
    if (tid == 0) { ctl.n = fr.z ? 0u : N; ctl.n_fg = 0u; }
    __syncthreads();
    if (fr.z || quota) {
        uint32_t c = 0, cf = 0;
        for (uint32_t i = tid; i < N; i += kSubT) {
            if (!survives(fr, i)) continue;
            ++c;
            if (quota && fr.cls[i] != 0) ++cf;
        }
        c = (uint32_t)wave_sum_i((int)c);
        cf = (uint32_t)wave_sum_i((int)cf);
        if (lane_id() == 0) {
            if (fr.z) atomicAdd(&ctl.n, c);
            atomicAdd(&ctl.n_fg, cf);
        }
        __syncthreads();
    }
    const uint32_t n = ctl.n, n_fg = ctl.n_fg, nb = (uint32_t)a.nb;
    uint32_t k_fg = 0;
    int st = SSF_SAMPLE_OK;
    if (n == 0) {
        st = SSF_SAMPLE_EMPTY;
    } else if (quota) {
        k_fg = min(min(n_fg, (uint32_t)a.quota), nb);
        if (n - n_fg < nb - k_fg) st = SSF_SAMPLE_SHORT;
    }
    if (tid == 0) { a.n_out[f] = (int32_t)n; a.status[f] = st; }
    if (st != SSF_SAMPLE_OK) {
        for (uint32_t j = tid; j < nb; j += kSubT) {
            idx[j] = 0;
            if (xyz) { xyz[j] = 0.0f; xyz[nb + j] = 0.0f; xyz[2 * nb + j] = 0.0f; }
        }
        return;
    }

    if (!quota && n <= nb) {
        // ---- with replacement: the survivors by index, slot j takes rank (key(1, j) n) >> 32 ----
        select_sorted(fr, kAll, false, N, n, sub_buf, ctl);
        for (uint32_t j = tid; j < nb; j += kSubT) {
            const uint32_t r = (uint32_t)(((uint64_t)key32(s1, j) * n) >> 32);
            const uint32_t i = (uint32_t)sub_buf[r];
            idx[j] = (int32_t)i;
            if (xyz) {
                const float* p = pts + (int64_t)i * a.stride;
                xyz[j] = p[0]; xyz[nb + j] = p[1]; xyz[2 * nb + j] = p[2];
            }
        }
        return;
    }
    // ---- without replacement: one part, or the foreground part then the background part ----
    uint32_t o = 0;
    for (int part = 0; part < 2; ++part) {
        const int kind = quota ? (part == 0 ? kFg : kBg) : kAll;
        const uint32_t m = quota ? (part == 0 ? k_fg : nb - k_fg) : (part == 0 ? nb : 0u);
        if (m == 0) continue;
        select_sorted(fr, kind, true, N, m, sub_buf, ctl);
        for (uint32_t j = tid; j < m; j += kSubT) {
            const uint32_t i = (uint32_t)sub_buf[j];
            idx[o + j] = (int32_t)i;
            if (xyz) {
                const float* p = pts + (int64_t)i * a.stride;
                xyz[o + j] = p[0]; xyz[nb + o + j] = p[1]; xyz[2 * nb + o + j] = p[2];
            }
        }
        o += m;
        __syncthreads();                        // the buffer is the next part's histogram
    }
}

hipError_t launch_subsample(hipStream_t s, int n_frames, const float* pts, int stride,
                            const int64_t* frame_off, const uint8_t* cls, int nb, float z_min,
                            int use_z, int quota, uint64_t seed, const uint64_t* h_tag, int key_bits,
                            int32_t* idx, float* xyz, int32_t* n_out, int32_t* status) {
    if (n_frames <= 0) return hipSuccess;
    static hipError_t once = hipFuncSetAttribute((const void*)k_subsample,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSubLds);
    if (once != hipSuccess) return once;
    SubArgs a;
    a.pts = pts; a.off = frame_off; a.cls = cls; a.idx = idx; a.xyz = xyz; a.n_out = n_out;
    a.status = status; a.seed = seed; a.stride = stride; a.nb = nb; a.use_z = use_z ? 1 : 0;
    a.quota = quota; a.key_bits = key_bits; a.z_min = z_min;
    SubTags tags = {};
    if (!h_tag) {                               // tag = the frame's position: one launch
        a.frame0 = 0; a.use_tags = 0;
        kmark(s, "k_subsample");
        hipLaunchKernelGGL(k_subsample, dim3(n_frames), dim3(kSubT), kSubLds, s, a, tags);
        return hipGetLastError();
    }
    // the tags ride in the kernel arguments (no staging buffer, nothing to outlive the call):
    // SSF_SAMPLE_TAG_CHUNK frames per launch
    for (int f0 = 0; f0 < n_frames; f0 += SSF_SAMPLE_TAG_CHUNK) {
        const int nf = n_frames - f0 < SSF_SAMPLE_TAG_CHUNK ? n_frames - f0 : SSF_SAMPLE_TAG_CHUNK;
        for (int k = 0; k < nf; ++k) tags.t[k] = h_tag[f0 + k];
        a.frame0 = f0; a.use_tags = 1;
        kmark(s, "k_subsample");
        hipLaunchKernelGGL(k_subsample, dim3(nf), dim3(kSubT), kSubLds, s, a, tags);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace ssf
