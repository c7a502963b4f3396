// feat_select.hip -- the frame kernels of the single-read feature stage, after the chunk kernels
// (feat_wave.hip, feat_chunk.hip) left their chunk-major counts, positions and bit planes:
//   k_feat_select  the frame's candidates in ring order, the unresolved points decided, the
//                  greedy spacing rule (frameFeature.cpp:110-123), the plane (and edge) clouds
//   k_feat_debug   debug outputs only: the ring-ordered cloud and every curvature
#include "feat_common.hpp"

namespace ssf {

// k_feat_select: one 1024-thread work-group per frame.  The chunks' row counts become, in LDS,
// each row's base per chunk (exclusive prefix over chunks: indexInRow of the segment's first
// point; the row lengths n_r and the ring offsets follow) and each segment's start in its chunk's
// own-tile order (exclusive prefix over rows).  Every (chunk, row) segment of the candidate planes
// is then copied, 64 bits at a time, to its row's place in ring order (bit ro[r] + indexInRow):
// the frame's candidates as row-major bit words in LDS, as k_select had them.  The unresolved
// points are decided (row ends -> curvature 0, :85; open stencils evaluated through the
// chunk-major index, the same taps in the same order) and OR-ed in; then the greedy spacing rule
// (:110-123) with one row per lane of wave 0 (wave 1: the edge rule), count-trailing-zeros walks
// over the row's words; each selection is stored as its chunk-major slot (the walk tracks the
// chunk its indexInRow falls in).  After a row prefix every thread emits framePlanePtr-ordered
// output: the point gathered through the slot's index, intensity = indexInRow + row / 100.0 (:77).
constexpr int kFeatRowWords = kFeatMaxChunks * kFeatWords + 1;   // ring-order words of a frame (+1)

template <bool kEdge>
__global__ __launch_bounds__(kSelThreads) void k_feat_select(const float* __restrict__ pts, int stride,
                                                             const int64_t* __restrict__ frame_off,
                                                             int n_rows, int n_chunks, int row_start,
                                                             int row_end, int plane_span,
                                                             float plane_min, float edge_min,
                                                             int32_t* __restrict__ cnt,
                                                             const uint16_t* __restrict__ gidx,
                                                             const uint64_t* __restrict__ gbits,
                                                             int32_t* __restrict__ ring_off,
                                                             float* __restrict__ curv_cm,
                                                             int32_t* __restrict__ sel,
                                                             float4* __restrict__ plane,
                                                             int32_t* __restrict__ plane_count,
                                                             int edge_span, int32_t* __restrict__ esel,
                                                             float4* __restrict__ edge,
                                                             int32_t* __restrict__ edge_count,
                                                             const uint8_t* __restrict__ irregular,
                                                             const uint8_t* __restrict__ lanemap) {
    constexpr int kRB = kFeatMaxChunks + 1;                   // odd stride: conflict-free columns
    __shared__ int rb[kMaxRows][kRB];                         // row base per chunk; [.][ncf] = n_r
    __shared__ uint16_t ss[kFeatMaxChunks][kMaxRows];         // segment start in the chunk's slots
    __shared__ uint64_t wl[kEdge ? 2 : 1][kFeatRowWords];     // candidates in ring order
    // one chunk-major candidate plane staged from global (coalesced) for the transposition, then
    // reused for the planar selections (indexInRow per output slot) when they fit
    __shared__ uint64_t stg[kFeatMaxChunks * kFeatWords];
    __shared__ int ro[kMaxRows + 1];
    __shared__ int lb[kMaxRows + 1];                          // per-row slot bases of the LDS selections
    __shared__ int pre[2][kMaxRows + 1];
    // per chunk: 1 = general-kernel block (positions from the u16 index), else its row -> lane map
    // (k_feat_wave_reg: a selected point's chunk position is 64 x its own column + that lane)
    __shared__ uint8_t irc[kFeatMaxChunks];
    __shared__ uint8_t lmc[kFeatMaxChunks][kMaxRows];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int nwv = kSelThreads / 64;
    const int f = blockIdx.x;
    const int64_t fb = frame_off[f];
    const int nf = (int)(frame_off[f + 1] - fb);
    const int ncf = (nf + kBinChunk - 1) / kBinChunk;
    int32_t* C = cnt + (int64_t)f * (n_chunks + 1) * kMaxRows;
    const uint64_t* Bf = gbits + (int64_t)f * n_chunks * (kFeatPlanes * kFeatWords);
    const uint16_t* GI = gidx + idx_base(frame_off, f);
    // every global load of the set-up issued first, into registers (one latency, not one per
    // loop trip): the chunks' row counts (a wave's chunks), their candidate and unresolved words,
    // the block flags and the lane maps (4-byte words)
    constexpr int kCPW = kFeatMaxChunks / nwv;                // chunks per wave at most
    constexpr int kWPT = kFeatMaxChunks * kFeatWords / kSelThreads;   // plane words per thread
    constexpr int kLPT = kFeatMaxChunks * kMaxRows / 4 / kSelThreads; // lane-map words per thread
    int cv[kCPW];
#pragma unroll
    for (int i = 0; i < kCPW; ++i) {
        const int c = w + i * nwv;
        cv[i] = c < ncf ? C[c * kMaxRows + lane] : 0;
    }
    uint64_t pwd[kWPT], uwd[kWPT];
#pragma unroll
    for (int i = 0; i < kWPT; ++i) {
        const int k = tid + i * kSelThreads, cc = k / kFeatWords, wi = k - cc * kFeatWords;
        const bool in = k < ncf * kFeatWords;
        pwd[i] = in ? Bf[cc * (kFeatPlanes * kFeatWords) + wi] : 0ull;
        uwd[i] = in ? Bf[cc * (kFeatPlanes * kFeatWords) + kFeatWords + wi] : 0ull;
    }
    uint32_t lmw[kLPT];
    const uint32_t* LM = reinterpret_cast<const uint32_t*>(lanemap + (lanemap ? (int64_t)f * n_chunks * kMaxRows : 0));
#pragma unroll
    for (int i = 0; i < kLPT; ++i) {
        const int k = tid + i * kSelThreads;
        lmw[i] = (lanemap && k < ncf * (kMaxRows / 4)) ? LM[k] : 0u;
    }
    const uint8_t irv = (tid < ncf && irregular) ? irregular[(int64_t)f * n_chunks + tid] : (uint8_t)1;
    if (tid < ncf) irc[tid] = irv;
#pragma unroll
    for (int i = 0; i < kLPT; ++i) {
        const int k = tid + i * kSelThreads;
        if (k < ncf * (kMaxRows / 4)) reinterpret_cast<uint32_t*>(&lmc[0][0])[k] = lmw[i];
    }
    // the frame-local input index of row r's point j (indexInRow) in chunk cc (rb: row bases)
    auto point_of = [&](int cc, int r, int j) -> int {
        const int o = j - rb[r][cc];                          // its place in the (chunk, row) segment
        const uint8_t m = irc[cc];
        return cc * kBinChunk + (m == kIrrRun ? (int)GI[(int64_t)cc * kBinChunk + r] + o
                                 : m ? (int)GI[(int64_t)cc * kBinChunk + ss[cc][r] + o] : 64 * o + lmc[cc][r]);
    };
    // counts -> segment starts (prefix over rows, per chunk); counts into rb
#pragma unroll
    for (int i = 0; i < kCPW; ++i) {
        const int c = w + i * nwv;
        if (c >= ncf) break;                                  // uniform
        const int v = cv[i];
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        ss[c][lane] = (uint16_t)(incl - v);
        rb[lane][c] = v;
    }
    const int nwf = (nf + 63) / 64 + 1;                       // ring-order words of this frame
    for (int k = tid; k < nwf; k += kSelThreads) {
        wl[0][k] = 0ull;
        if (kEdge) wl[kEdge ? 1 : 0][k] = 0ull;
    }
    __syncthreads();
    for (int r = w; r < kMaxRows; r += nwv) {                 // per row: prefix over the chunks
        int carry = 0;
        for (int c0 = 0; c0 < ncf; c0 += 64) {                // uniform
            const int c = c0 + lane;
            const int v = c < ncf ? rb[r][c] : 0;
            int incl = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(incl, o, 64);
                if (lane >= o) incl += y;
            }
            if (c < ncf) rb[r][c] = carry + incl - v;
            carry += __shfl(incl, 63, 64);
        }
        if (lane == 0) rb[r][ncf] = carry;
    }
    __syncthreads();
    if (tid < 64) {                                           // ring offsets: prefix over rows
        const int nr = tid < n_rows ? rb[tid][ncf] : 0;
        int incl = nr;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o, 64);
            if (tid >= o) incl += y;
        }
        if (tid < n_rows) ro[tid] = incl - nr;
        if (tid == 63) ro[n_rows] = incl;
        // a row of n_r points makes at most ceil(n_r / planeSpan) selections: slot bases for
        // the LDS copy of the planar selections
        const int cap = tid < n_rows ? (nr + plane_span - 1) / max(1, plane_span) : 0;
        int ci = cap;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(ci, o, 64);
            if (tid >= o) ci += y;
        }
        if (tid < n_rows) lb[tid] = ci - cap;
        if (tid == 63) lb[n_rows] = ci;
    }
    __syncthreads();
    if (tid <= n_rows) ring_off[(int64_t)f * (n_rows + 1) + tid] = ro[tid];
    if (curv_cm)                                              // debug: the row bases for k_feat_debug
        for (int k = tid; k < (ncf + 1) * kMaxRows; k += kSelThreads)
            C[k] = rb[k % kMaxRows][k / kMaxRows];
    // candidate planes: every (chunk, row) segment of a row in range to its ring-order bits,
    // one plane at a time through the staging copy
#pragma unroll
    for (int pl = 0; pl < (kEdge ? 2 : 1); ++pl) {
        if (pl) __syncthreads();                              // the previous plane's reads are done
        if (pl == 0) {
#pragma unroll
            for (int i = 0; i < kWPT; ++i) {
                const int k = tid + i * kSelThreads;
                if (k < ncf * kFeatWords) stg[k] = pwd[i];
            }
        } else {
            for (int k = tid; k < ncf * kFeatWords; k += kSelThreads) {
                const int c = k / kFeatWords, wi = k - c * kFeatWords;
                stg[k] = Bf[c * (kFeatPlanes * kFeatWords) + 2 * kFeatWords + wi];
            }
        }
        __syncthreads();
        for (int k = tid; k < ncf * kMaxRows; k += kSelThreads) {
            const int c = k / kMaxRows, r = k - c * kMaxRows;
            if (r < row_start || r >= n_rows - row_end) continue;
            const int L = rb[r][c + 1] - rb[r][c];
            const int src0 = c * kBinChunk + ss[c][r], dst0 = ro[r] + rb[r][c];
            for (int b = 0; b < L; b += 64) {
                const int sb = src0 + b, wi = sb >> 6, sh = sb & 63;
                uint64_t v = stg[wi] >> sh;
                if (sh && wi + 1 < ncf * kFeatWords) v |= stg[wi + 1] << (64 - sh);
                const int nb = L - b;
                if (nb < 64) v &= (1ull << nb) - 1ull;
                if (!v) continue;
                const int db = dst0 + b, di = db >> 6, dh = db & 63;
                atomicOr((unsigned long long*)&wl[pl][di], v << dh);
                if (dh) atomicOr((unsigned long long*)&wl[pl][di + 1], v >> (64 - dh));
            }
        }
    }
    // the unresolved own points of rows in range
#pragma unroll
    for (int i = 0; i < kWPT; ++i) {
        const int k = tid + i * kSelThreads;
        const int c = k / kFeatWords, wi = k - c * kFeatWords;
        uint64_t u = uwd[i];                                  // 0 beyond the frame's words
        while (u) {
            const int p = 64 * wi + (int)__builtin_ctzll(u);
            u &= u - 1ull;
            int r = 0;                                        // the last row whose segment starts <= p
#pragma unroll
            for (int st = 32; st > 0; st >>= 1)
                if (r + st < kMaxRows && ss[c][r + st] <= p) r += st;
            const int j = rb[r][c] + (p - ss[c][r]), nr = rb[r][ncf];
            const int g = ro[r] + j;                          // ring position
            if (j < 5 || j >= nr - 5) {                       // curvature 0: a planar candidate
                atomicOr((unsigned long long*)&wl[0][g >> 6], 1ull << (g & 63));
                continue;
            }
            float ux[11], uy[11], uz[11];                     // an open stencil, through the index
#pragma unroll
            for (int m = 0; m < 11; ++m) {
                const int jj = j - 5 + m;
                int cc = 0;                                   // the last chunk whose base <= jj
                for (int st = 64; st > 0; st >>= 1)
                    if (cc + st < ncf && rb[r][cc + st] <= jj) cc += st;
                const int ii = point_of(cc, r, jj);
                const float* q = pts + (fb + ii) * stride;
                ux[m] = q[0]; uy[m] = q[1]; uz[m] = q[2];
            }
            const float d0 = tap11(ux), d1 = tap11(uy), d2 = tap11(uz);
            float val = d0 * d0 + d1 * d1;
            val = val + d2 * d2;
            const uint8_t fl = cand_flags(true, true, val, plane_min, kEdge, edge_min);
            if (fl & 1) atomicOr((unsigned long long*)&wl[0][g >> 6], 1ull << (g & 63));
            if (kEdge && (fl & 2)) atomicOr((unsigned long long*)&wl[kEdge ? 1 : 0][g >> 6], 1ull << (g & 63));
            if (curv_cm) curv_cm[fb + (int64_t)c * kBinChunk + p] = val;
        }
    }
    __syncthreads();
    // the planar selections (indexInRow per slot) stay in LDS when a frame cannot make more than
    // the staging region holds (sum over rows of ceil(n_r / span) <= nf / span + rows)
    const bool sel_lds = lb[n_rows] <= kFeatMaxChunks * kFeatWords * 2;
    int32_t* sel_l = reinterpret_cast<int32_t*>(stg);
    if (w < (kEdge ? 2 : 1)) {                                // wave 0 planes, wave 1 edges
        const int r = lane;
        const bool e = kEdge && w == 1;
        const uint64_t* W = wl[e ? 1 : 0];
        const int span = e ? edge_span : plane_span;
        const bool lds_out = !e && sel_lds;
        int32_t* out = e ? esel + fb : (lds_out ? sel_l : sel + fb);
        int cnt_r = 0;
        if (r < n_rows && r >= row_start && r < n_rows - row_end) {
            const int rs = ro[r], n_r = ro[r + 1] - rs;
            if (n_r > 0) {
                int js = 0;                                   // jstart, row-relative
                const int kend = (rs + n_r - 1) >> 6;
                int32_t* orow = out + (lds_out ? lb[r] : rs);  // this row's selection slots
                uint64_t nxt = W[rs >> 6];
                for (int k = rs >> 6; k <= kend; ++k) {       // the row's words in order
                    uint64_t wv = nxt;
                    nxt = W[min(k + 1, kend)];                // the next word in flight
                    const int gb = k * 64;
                    int low = rs + js - gb;
                    if (low >= 64) continue;
                    if (low > 0) wv &= ~0ull << low;
                    const int top = rs + n_r - gb;
                    if (top < 64) wv &= (1ull << top) - 1ull;
                    while (wv) {
                        const int j = gb + (int)__builtin_ctzll(wv) - rs;
                        orow[cnt_r] = j;                      // indexInRow
                        ++cnt_r;
                        js = j + span;
                        low = rs + js - gb;
                        wv = low >= 64 ? 0ull : (wv & (~0ull << low));
                    }
                }
            }
        }
        int incl = cnt_r;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane < n_rows) pre[e ? 1 : 0][lane] = incl - cnt_r;
        if (lane == 63) pre[e ? 1 : 0][n_rows] = incl;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < (kEdge ? 2 : 1); ++e) {
        const int* P = pre[e];
        const int total = P[n_rows];
        if (tid == 0) (e ? edge_count : plane_count)[f] = total;
        const bool lds_in = !e && sel_lds;
        const int32_t* S = e ? esel + fb : (lds_in ? sel_l : sel + fb);
        const int* SB = lds_in ? lb : ro;                     // per-row slot bases
        float4* O = e ? edge : plane;
        constexpr int U = SSF_SEL_OUT_U;          // outputs per thread per trip (loads in flight)
        for (int k0 = 0; k0 < total; k0 += U * kSelThreads) {   // uniform
            int kk[U], rr[U], jj[U], ii[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                kk[u] = min(k0 + u * kSelThreads + tid, total - 1);
                int a = 0;
#pragma unroll
                for (int st = 32; st > 0; st >>= 1)
                    if (a + st < n_rows && P[a + st] <= kk[u]) a += st;
                rr[u] = a;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) jj[u] = S[SB[rr[u]] + (kk[u] - P[rr[u]])];
#pragma unroll
            for (int u = 0; u < U; ++u) {                     // indexInRow -> chunk, slot, position
                const int r = rr[u], j = jj[u];
                int cc = 0;                                   // the last chunk whose base <= j
#pragma unroll
                for (int st = 64; st > 0; st >>= 1)
                    if (cc + st < ncf && rb[r][cc + st] <= j) cc += st;
                ii[u] = point_of(cc, r, j);
            }
            float q[U][3];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float* p = pts + (fb + ii[u]) * stride;
                q[u][0] = p[0]; q[u][1] = p[1]; q[u][2] = p[2];
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (k0 + u * kSelThreads + tid < total)
                    O[fb + kk[u]] = make_float4(q[u][0], q[u][1], q[u][2],
                                                (float)((double)jj[u] + (double)rr[u] / 100.0));
        }
    }
}

// Parity outputs of the single-read stage (debug only): per own-tile slot of a chunk, its row and
// indexInRow from the row bases k_feat_select left in cnt, and at its ring position the point
// (x, y, z, intensity = indexInRow + row / 100.0) and its curvature (chunk-major -> ring order).
__global__ __launch_bounds__(256) void k_feat_debug(const float* __restrict__ pts, int stride,
                                                    const int64_t* __restrict__ frame_off,
                                                    int n_rows, int n_chunks,
                                                    const int32_t* __restrict__ cnt,
                                                    const int32_t* __restrict__ ring_off,
                                                    const uint16_t* __restrict__ gidx,
                                                    const float* __restrict__ curv_cm,
                                                    float4* __restrict__ out4, float* __restrict__ curv) {
    __shared__ int base[kMaxRows], segs[kMaxRows + 1], ro[kMaxRows];
    const int c = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const int64_t fb = frame_off[f];
    const int nf = (int)(frame_off[f + 1] - fb);
    if ((int64_t)c * kBinChunk >= nf) return;
    const int32_t* Cb = cnt + (int64_t)f * (n_chunks + 1) * kMaxRows;
    if (tid < 64) {
        const int b0 = Cb[c * kMaxRows + tid], b1 = Cb[(c + 1) * kMaxRows + tid];
        const int v = b1 - b0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o, 64);
            if (tid >= o) incl += y;
        }
        base[tid] = b0;
        segs[tid] = incl - v;
        if (tid == 63) segs[64] = incl;
        ro[tid] = tid < n_rows ? ring_off[(int64_t)f * (n_rows + 1) + tid] : 0;
    }
    __syncthreads();
    const int no = segs[64];
    const uint16_t* GI = gidx + idx_base(frame_off, f) + (int64_t)c * kBinChunk;
    for (int p = tid; p < no; p += 256) {
        int r = 0;
#pragma unroll
        for (int st = 32; st > 0; st >>= 1)
            if (r + st < kMaxRows && segs[r + st] <= p) r += st;
        const int j = base[r] + (p - segs[r]);
        const int64_t g = fb + ro[r] + j;
        const int ii = c * kBinChunk + (int)GI[p];
        const float* q = pts + (fb + ii) * stride;
        if (out4) out4[g] = make_float4(q[0], q[1], q[2], (float)((double)j + (double)r / 100.0));
        if (curv) curv[g] = curv_cm[fb + (int64_t)c * kBinChunk + p];
    }
}

void launch_feat_select(const FeatLaunch& a, const FeatScratch& fs) {
    const FeatFrames& in = a.in;
    const ssf_config& cfg = a.cfg;
    kmark(a.s, "k_feat_select");
    dispatch_de(false, a.edge, [&](auto, auto E) {
        hipLaunchKernelGGL(k_feat_select<decltype(E)::value>, dim3(a.n_frames), dim3(kSelThreads), 0, a.s,
                           in.pts, in.stride, in.frame_off, cfg.n_rows, a.n_chunks, cfg.row_start, cfg.row_end,
                           cfg.plane_span, cfg.plane_min, a.es.min_curv, fs.cnt, fs.gidx, fs.gbits,
                           a.out.ring_off, fs.curv_cm, a.sel, a.out.plane, a.out.plane_count, a.es.span,
                           a.es.sel, a.es.out, a.es.count, fs.irr, fs.lmap);
    });
}

void launch_feat_debug(const FeatLaunch& a, const FeatScratch& fs) {
    kmark(a.s, "k_feat_debug");
    hipLaunchKernelGGL(k_feat_debug, dim3(a.n_chunks, a.n_frames), dim3(256), 0, a.s, a.in.pts, a.in.stride,
                       a.in.frame_off, a.cfg.n_rows, a.n_chunks, fs.cnt, a.out.ring_off, fs.gidx, fs.curv_cm,
                       a.out.ring_xyzi, a.out.curv);
}

}  // namespace ssf
