// The cost volume of the TFlow scene-flow network for gfx950: the three kernels under
// PointConvTransFlowV2.forward (scripts/ActiveSceneFlow/utils/soflow.py:354-525), DESIGN.md §6.10.
//
//   k_grouped_mlp          <- the grouped MLPs mlp_convs, mlp_convs2, mlp_convs3, mlp_convs4 and
//                             weightnet1 (:392-418, :424-451, :460-461, :489-509): the kernel of
//                             §6.9 (k_grouped_mlp_max, pointnet2.hip) with a four-segment input
//                             column, a per-layer leaky slope and a second output mode
//   k_pair_attention       <- the k x k mutual attention (:420-422, :453-458)
//   k_segment_softmax_sum  <- softmax over the samples and the weighted sum (:469, :486), and
//                             torch_scatter's scatter_softmax, product and scatter_sum (:471-481)
//
// All float32, no float atomics, no allocation; sums run in a fixed order (fma chains), so a batch
// element has the same bits alone, in any batch and from run to run.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ssf_device.hpp"
#include "mlp_tile.hpp"
#include "../../include/ssf_pointnet2.h"

namespace {

using ssf_pn2_detail::fail;
using ssf_pn2_detail::hip_status;

constexpr int kGmlpMaxN = 36864;               // the bound of ssf_pn2_grouped_mlp_max on n

// ------------------------------------------------------------------------------------------
// k_grouped_mlp: the layout, tile walk and LDS images of k_grouped_mlp_max (pointnet2.hip).  The
// input column of centroid j, sample m is cat(ctr[:, j], feat[:, i], dense[:, j, m],
// xyz[:, i] - new_xyz[:, j]) with i = idx[j, m]; a layer is t = fmaf(sum, scale, shift),
// y = t > 0 ? t : slope * t.  The last layer's tile either goes through the per-wave staging patch
// for the max over k, or straight from the accumulators to d_out [b, w, s, k]: the columns of a
// 32-column tile are consecutive (j, m) pairs, so a row of the tile is one contiguous store.
struct GmlpArgs {
    const float* ctr;
    const float* feat;
    const float* dense;
    const float* xyz;
    const float* new_xyz;
    const int32_t* idx;
    const float* wt[SSF_PN2_MLP_MAX_LAYERS];
    const float* scale[SSF_PN2_MLP_MAX_LAYERS];
    const float* shift[SSF_PN2_MLP_MAX_LAYERS];
    float slope[SSF_PN2_MLP_MAX_LAYERS];
    float* out;
    int32_t* bad;
    int32_t width[SSF_PN2_MLP_MAX_LAYERS + 1];
    int32_t n, s, k, c_ctr, c_g, c_d, n_layers, tc, buf1, full;
};

__global__ __launch_bounds__(kMlpThreads) void k_grouped_mlp(const GmlpArgs A) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, tc = A.tc, k = A.k, n = A.n, s = A.s;
    const int cpt = 32 / k, ct = tc >> 5;                      // centroids per tile, tiles
    const int j0 = blockIdx.x * (cpt * ct);                    // first centroid of the block
    int32_t* sidx = reinterpret_cast<int32_t*>(mlp_lds) + (A.buf1 - 2 * tc);   // [tc] index, [tc] centroid

    // the block's index list: -1 marks an unused column (0 stands for "no gather" without d_idx)
    for (int col = tid; col < tc; col += kMlpThreads) {
        const int t = col >> 5, w = col & 31, q = w / k, m = w - q * k;
        const int j = j0 + t * cpt + q;
        int i = -1;
        if (q < cpt && j < s) {
            i = 0;
            if (A.idx) {
                i = A.idx[((int64_t)b * s + j) * k + m];
                if ((unsigned)i >= (unsigned)n) { *A.bad = 1; i = 0; }
            }
        }
        sidx[col] = i;
        sidx[tc + col] = j;
    }
    __syncthreads();
    const int w0 = A.width[0];
    const int c1 = A.c_ctr, c2 = c1 + A.c_g, c3 = c2 + A.c_d;  // segment ends
    const float* CT = A.ctr ? A.ctr + (int64_t)b * A.c_ctr * s : nullptr;
    const float* FT = A.feat ? A.feat + (int64_t)b * A.c_g * n : nullptr;
    const float* DN = A.dense ? A.dense + (int64_t)b * A.c_d * s * k : nullptr;
    const float* XY = A.xyz ? A.xyz + (int64_t)b * 3 * n : nullptr;
    const float* NX = A.new_xyz ? A.new_xyz + (int64_t)b * 3 * s : nullptr;
    for (int e = tid; e < w0 * tc; e += kMlpThreads) {
        const int ch = e / tc, col = e - ch * tc;
        const int i = sidx[col];
        float v = 0.0f;
        if (i >= 0) {
            const int j = sidx[tc + col];
            if (ch < c1) v = CT[(int64_t)ch * s + j];
            else if (ch < c2) v = FT[(int64_t)(ch - c1) * n + i];
            else if (ch < c3) {
                const int w = col & 31, m = w - (w / k) * k;
                v = DN[((int64_t)(ch - c2) * s + j) * k + m];
            } else v = XY[(ch - c3) * n + i] - NX[(ch - c3) * s + j];
        }
        mlp_lds[e] = v;
    }
    __syncthreads();

    const int r = lane & 31, h = lane >> 5;
    for (int l = 0; l < A.n_layers; ++l) {
        const int w_in = A.width[l], w_out = A.width[l + 1];
        const int x0 = (l & 1) ? A.buf1 : 0, y0 = (l & 1) ? 0 : A.buf1;
        const bool last = l + 1 == A.n_layers;
        const int ot = (w_out + 31) >> 5;
        const int st0 = y0 + wave * kMlpStage;                 // the wave's staging patch
        const float* __restrict__ SC = A.scale[l];
        const float* __restrict__ SH = A.shift[l];
        const float sl = A.slope[l];
        for (int p = wave; p < ot * ct; p += kMlpWaves) {
            const int o0 = (p / ct) << 5, c0 = (p % ct) << 5;
            const f16v acc = mlp_tile(A.wt[l], w_in, w_out, o0, x0, tc, c0, lane);
            const int jt = j0 + (c0 >> 5) * cpt;               // first centroid of this tile
            // C/D map of the 32x32 MFMA: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
                const int o = o0 + row;
                const int oc = o < w_out ? o : w_out - 1;
                const float t = __builtin_fmaf(acc[i], SC[oc], SH[oc]);
                const float y = t > 0.0f ? t : sl * t;
                if (last && A.full) {
                    // column r of the tile is entry jt * k + r of the row's [s, k] plane
                    if (o < w_out && r < cpt * k && jt + r / k < s)
                        A.out[((int64_t)b * w_out + o) * s * k + (int64_t)jt * k + r] = y;
                } else if (last) mlp_lds[st0 + row * 33 + r] = y;
                else if (o < w_out) mlp_lds[y0 + o * tc + c0 + r] = y;
            }
            if (last && !A.full) {
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                __builtin_amdgcn_wave_barrier();
                // the max over the k samples: 32 rows x cpt centroids of this tile
                for (int e = lane; e < 32 * cpt; e += 64) {
                    const int row = e / cpt, q = e - row * cpt;
                    const int o = o0 + row, j = jt + q;
                    if (o < w_out && j < s) {
                        const int s0 = st0 + row * 33 + q * k;
                        float mx = mlp_lds[s0];
                        for (int m = 1; m < k; ++m) mx = fmaxf(mx, mlp_lds[s0 + m]);
                        A.out[((int64_t)b * w_out + o) * s + j] = mx;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// k_pair_attention (soflow.py:420-422, :453-458): one work-group per centroid.  LDS holds the
// centroid's two c x k blocks (rows padded to an odd length kp), the k x k logits a and weights W,
// and the 4 k softmax statistics.  a[m][m'] = sum_ch q[ch][m] kw[ch][m'] (ch ascending);
// W = softmax over m (torch.softmax(., -2)) times softmax over m' (., -1); qm = q + W kw^T,
// kwm = kw + q W.
constexpr int kAttnThreads = 256;

int attn_lds_floats(int c, int k) {               // the kernel lays the same regions out itself
    const int kp = k | 1;
    return 2 * c * kp + 2 * k * kp + 4 * k;
}

__global__ __launch_bounds__(kAttnThreads) void k_pair_attention(const float* __restrict__ q,
                                                                 const float* __restrict__ kw,
                                                                 float* __restrict__ qm,
                                                                 float* __restrict__ kwm, int c,
                                                                 int s, int k) {
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int kp = k | 1;
    float* Q = mlp_lds;
    float* KW = Q + c * kp;
    float* Am = KW + c * kp;
    float* Wm = Am + k * kp;
    float* rmax = Wm + k * kp;                     // over m' for a fixed m
    float* rsum = rmax + k;
    float* cmax = rsum + k;                        // over m for a fixed m'
    float* csum = cmax + k;
    const int64_t cs = (int64_t)s * k;
    const int64_t base = (int64_t)b * c * cs + (int64_t)j * k;
    for (int e = tid; e < c * k; e += kAttnThreads) {
        const int ch = e / k, m = e - ch * k;
        Q[ch * kp + m] = q[base + ch * cs + m];
        KW[ch * kp + m] = kw[base + ch * cs + m];
    }
    __syncthreads();
    for (int e = tid; e < k * k; e += kAttnThreads) {
        const int m = e / k, mp = e - m * k;
        float a = 0.0f;
        for (int ch = 0; ch < c; ++ch) a = __builtin_fmaf(Q[ch * kp + m], KW[ch * kp + mp], a);
        Am[m * kp + mp] = a;
    }
    __syncthreads();
    if (tid < 2 * k) {
        const bool row = tid < k;
        const int i = row ? tid : tid - k;
        const int i0 = row ? i * kp : i, st = row ? 1 : kp;
        float mx = Am[i0];
        for (int t = 1; t < k; ++t) mx = fmaxf(mx, Am[i0 + t * st]);
        float su = 0.0f;
        for (int t = 0; t < k; ++t) su += expf(Am[i0 + t * st] - mx);
        if (row) { rmax[i] = mx; rsum[i] = su; }
        else { cmax[i] = mx; csum[i] = su; }
    }
    __syncthreads();
    for (int e = tid; e < k * k; e += kAttnThreads) {
        const int m = e / k, mp = e - m * k;
        const float a = Am[m * kp + mp];
        Wm[m * kp + mp] = (expf(a - cmax[mp]) / csum[mp]) * (expf(a - rmax[m]) / rsum[m]);
    }
    __syncthreads();
    for (int e = tid; e < c * k; e += kAttnThreads) {
        const int ch = e / k, m = e - ch * k;
        float x = 0.0f, y = 0.0f;
        for (int t = 0; t < k; ++t) {
            x = __builtin_fmaf(Wm[m * kp + t], KW[ch * kp + t], x);
            y = __builtin_fmaf(Q[ch * kp + t], Wm[t * kp + m], y);
        }
        qm[base + ch * cs + m] = Q[ch * kp + m] + x;
        kwm[base + ch * cs + m] = KW[ch * kp + m] + y;
    }
}

// ------------------------------------------------------------------------------------------
// k_segment_softmax_sum: a work-group takes 64 segments x 64 channels of one batch element.  The
// first 64 threads find their segment's bounds, maximum and exponential sum (serial over the
// segment, whatever its length); then one thread per (segment, channel), segments along the lanes,
// walks the segment once more and accumulates w_e val[ch][e] in the segment's order.
constexpr int kSegThreads = 256;
constexpr int kSegTile = 64;
constexpr int kSegChannels = 64;

__global__ __launch_bounds__(kSegThreads) void k_segment_softmax_sum(
    const float* __restrict__ logit, const float* __restrict__ val, const int32_t* __restrict__ offsets,
    const int32_t* __restrict__ order, float* __restrict__ out, int32_t* __restrict__ bad, int c, int m,
    int t_n, int k) {
    __shared__ float smx[kSegTile], ssm[kSegTile];
    __shared__ int slo[kSegTile], shi[kSegTile];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int t0 = blockIdx.x * kSegTile, c0 = blockIdx.z * kSegChannels;
    const float* L = logit + (int64_t)b * m;
    const int32_t* O = order ? order + (int64_t)b * m : nullptr;
    auto entry = [&](int e) {
        if (!O) return e;
        const int o = O[e];
        return (unsigned)o < (unsigned)m ? o : 0;
    };
    if (tid < kSegTile) {
        const int t = t0 + tid;
        int lo = 0, hi = 0;
        if (t < t_n) {
            if (O) {
                const int32_t* F = offsets + (int64_t)b * (t_n + 1);
                lo = F[t]; hi = F[t + 1];
                if (lo < 0 || lo > m) { *bad = 1; lo = lo < 0 ? 0 : m; }
                if (hi < lo || hi > m) { *bad = 1; hi = hi < lo ? lo : m; }
            } else {
                lo = t * k; hi = lo + k;
            }
        }
        float mx = -__builtin_inff(), su = 0.0f;
        for (int e = lo; e < hi; ++e) {
            if (O && (unsigned)O[e] >= (unsigned)m) *bad = 1;
            mx = fmaxf(mx, L[entry(e)]);
        }
        for (int e = lo; e < hi; ++e) su += expf(L[entry(e)] - mx);
        slo[tid] = lo; shi[tid] = hi; smx[tid] = mx; ssm[tid] = su;
    }
    __syncthreads();
    const int nch = min(kSegChannels, c - c0);
    for (int p = tid; p < kSegTile * nch; p += kSegThreads) {
        const int tl = p & (kSegTile - 1), ch = c0 + (p >> 6);
        const int t = t0 + tl;
        if (t >= t_n) continue;
        const int lo = slo[tl], hi = shi[tl];
        const float mx = smx[tl], su = ssm[tl];
        const float* V = val + ((int64_t)b * c + ch) * m;
        float acc = 0.0f;
        for (int e = lo; e < hi; ++e) {
            const int ee = entry(e);
            acc = __builtin_fmaf(expf(L[ee] - mx) / su, V[ee], acc);
        }
        out[((int64_t)b * c + ch) * t_n + t] = acc;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
extern "C" {

int32_t ssf_pn2_grouped_mlp(void* stream, int32_t b, int32_t n, int32_t s, int32_t k, int32_t c_ctr,
                            int32_t c_g, int32_t c_d, const float* d_ctr, const float* d_feat,
                            const float* d_dense, const float* d_xyz, const float* d_new_xyz,
                            const int32_t* d_idx, int32_t n_layers, const int32_t* widths,
                            const float* const* d_wt, const float* const* d_scale,
                            const float* const* d_shift, const float* slope, int32_t full_output,
                            float* d_out, int32_t* d_bad) {
    if (b < 0 || b > 65535 || s < 0 || k <= 0 || k > SSF_PN2_KNN_MAX || c_ctr < 0 || c_g < 0 || c_d < 0)
        return fail(SSF_PN2_E_ARG, "grouped_mlp: bad arguments (0 <= b <= 65535, s >= 0, 0 < k <= 32, segment widths >= 0)");
    if (n_layers < 1 || n_layers > SSF_PN2_MLP_MAX_LAYERS)
        return fail(SSF_PN2_E_ARG, "grouped_mlp: need 1 <= n_layers <= 3");
    if ((c_ctr > 0 && !d_ctr) || (c_g > 0 && !d_feat) || (c_d > 0 && !d_dense) || (d_xyz && !d_new_xyz) ||
        !widths || !d_wt || !d_scale || !d_shift || !slope || !d_out || !d_bad)
        return fail(SSF_PN2_E_ARG, "grouped_mlp: null pointer");
    const bool gathers = c_g > 0 || d_xyz;
    if (gathers && (!d_idx || n <= 0 || n > kGmlpMaxN))
        return fail(SSF_PN2_E_ARG, "grouped_mlp: a gathered segment needs d_idx and 0 < n <= 36864");
    GmlpArgs a{};
    if (widths[0] < 1 || widths[0] > SSF_PN2_GMLP_MAX_IN)
        return fail(SSF_PN2_E_ARG, "grouped_mlp: widths[0] must be in [1, 766]");
    a.width[0] = widths[0];
    for (int l = 1; l <= n_layers; ++l) {
        if (widths[l] < 1 || widths[l] > SSF_PN2_MLP_MAX_WIDTH)
            return fail(SSF_PN2_E_ARG, "grouped_mlp: every output width must be in [1, 512]");
        a.width[l] = widths[l];
    }
    if ((int64_t)widths[0] != (int64_t)c_ctr + c_g + c_d + (d_xyz ? 3 : 0))
        return fail(SSF_PN2_E_ARG, "grouped_mlp: widths[0] != c_ctr + c_g + c_d + (d_xyz ? 3 : 0)");
    for (int l = 0; l < n_layers; ++l) {
        if (!d_wt[l] || !d_scale[l] || !d_shift[l]) return fail(SSF_PN2_E_ARG, "grouped_mlp: null layer pointer");
        a.wt[l] = d_wt[l]; a.scale[l] = d_scale[l]; a.shift[l] = d_shift[l]; a.slope[l] = slope[l];
    }
    if (b == 0 || s == 0) return SSF_PN2_OK;
    // LDS rows of the two ping-pong images and the column tile: the rule of ssf_pn2_grouped_mlp_max
    int rows[2] = {0, 0};
    for (int l = 0; l < n_layers; ++l) rows[l & 1] = max(rows[l & 1], widths[l]);
    int tc = 128, buf1 = 0;
    size_t bytes = 0;
    for (;; tc >>= 1) {
        int f[2] = {rows[0] * tc, rows[1] * tc};
        f[n_layers & 1] = max(f[n_layers & 1], kMlpWaves * kMlpStage);
        buf1 = f[0] + 2 * tc;
        bytes = ((size_t)buf1 + f[1]) * 4;
        if (bytes <= (size_t)kMlpLdsMax / 2 || tc == 32) break;
    }
    if (bytes > (size_t)kMlpLdsMax) return fail(SSF_PN2_E_ARG, "grouped_mlp: widths do not fit in LDS");
    static hipError_t once = hipFuncSetAttribute((const void*)k_grouped_mlp,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, kMlpLdsMax);
    if (once != hipSuccess) return hip_status(once, "grouped_mlp: LDS limit");
    a.ctr = c_ctr > 0 ? d_ctr : nullptr; a.feat = c_g > 0 ? d_feat : nullptr;
    a.dense = c_d > 0 ? d_dense : nullptr; a.xyz = d_xyz; a.new_xyz = d_xyz ? d_new_xyz : nullptr;
    a.idx = gathers ? d_idx : nullptr; a.out = d_out; a.bad = d_bad;
    a.n = gathers ? n : 1; a.s = s; a.k = k; a.c_ctr = c_ctr; a.c_g = c_g; a.c_d = c_d;
    a.n_layers = n_layers; a.tc = tc; a.buf1 = buf1; a.full = full_output ? 1 : 0;
    const int cpb = (32 / k) * (tc / 32);
    hipLaunchKernelGGL(k_grouped_mlp, dim3((s + cpb - 1) / cpb, b), dim3(kMlpThreads), bytes,
                       (hipStream_t)stream, a);
    return hip_status(hipGetLastError(), "k_grouped_mlp");
}

int32_t ssf_pn2_pair_attention(void* stream, int32_t b, int32_t c, int32_t s, int32_t k,
                               const float* d_q, const float* d_kw, float* d_qm, float* d_kwm) {
    if (b < 0 || b > 65535 || s < 0 || c < 1 || c > SSF_PN2_ATTN_MAX_C || k < 1 || k > SSF_PN2_KNN_MAX)
        return fail(SSF_PN2_E_ARG, "pair_attention: bad arguments (0 <= b <= 65535, s >= 0, 1 <= c <= 512, 1 <= k <= 32)");
    if (!d_q || !d_kw || !d_qm || !d_kwm) return fail(SSF_PN2_E_ARG, "pair_attention: null pointer");
    if (b == 0 || s == 0) return SSF_PN2_OK;
    static hipError_t once = hipFuncSetAttribute((const void*)k_pair_attention,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, kMlpLdsMax);
    if (once != hipSuccess) return hip_status(once, "pair_attention: LDS limit");
    const size_t bytes = (size_t)attn_lds_floats(c, k) * 4;      // at most 144,128 B (c = 512, k = 32)
    hipLaunchKernelGGL(k_pair_attention, dim3(s, b), dim3(kAttnThreads), bytes, (hipStream_t)stream, d_q,
                       d_kw, d_qm, d_kwm, c, s, k);
    return hip_status(hipGetLastError(), "k_pair_attention");
}

int32_t ssf_pn2_segment_softmax_sum(void* stream, int32_t b, int32_t c, int32_t m, int32_t t_n,
                                    int32_t k, const float* d_logit, const float* d_val,
                                    const int32_t* d_offsets, const int32_t* d_order, float* d_out,
                                    int32_t* d_bad) {
    if (b < 0 || b > 65535 || c < 0 || c > 65535 * kSegChannels || m < 0 || t_n < 0)
        return fail(SSF_PN2_E_ARG, "segment_softmax_sum: bad arguments (0 <= b <= 65535, c, m, t_n >= 0)");
    if ((d_offsets == nullptr) != (d_order == nullptr))
        return fail(SSF_PN2_E_ARG, "segment_softmax_sum: CSR segments need both d_offsets and d_order");
    if (!d_order && (k < 1 || (int64_t)t_n * k != (int64_t)m))
        return fail(SSF_PN2_E_ARG, "segment_softmax_sum: uniform segments need k >= 1 and m = t_n * k");
    if (!d_logit || !d_val || !d_out || !d_bad) return fail(SSF_PN2_E_ARG, "segment_softmax_sum: null pointer");
    if (b == 0 || c == 0 || t_n == 0) return SSF_PN2_OK;
    const dim3 grid((t_n + kSegTile - 1) / kSegTile, b, (c + kSegChannels - 1) / kSegChannels);
    hipLaunchKernelGGL(k_segment_softmax_sum, grid, dim3(kSegThreads), 0, (hipStream_t)stream, d_logit,
                       d_val, d_offsets, d_order, d_out, d_bad, c, m, t_n, k);
    return hip_status(hipGetLastError(), "k_segment_softmax_sum");
}

}  // extern "C"
