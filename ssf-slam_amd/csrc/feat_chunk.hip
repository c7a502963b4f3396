// feat_chunk.hip -- the general chunk kernel of the single-read feature stage: k_feat_chunk (every
// chunk of the launch) and k_feat_chunk_flagged (the chunks the wave kernels of feat_wave.hip left
// flagged kIrrGeneral).  It takes any input order, and it defines the stage's outputs, which the
// wave kernels reproduce for the layouts they know.
// The single-read stage (these kernels, then k_feat_select) stands in for k_bin_count,
// k_bin_scan, k_bin_curv and k_select for frames of up to kFeatMaxChunks chunks.  The points are
// read ONCE: k_feat_chunk computes the ring ids of its window itself, ranks and regroups it by row
// exactly like k_bin_curv, and evaluates every stencil the window covers -- but it needs no global
// ring position: its outputs are CHUNK-MAJOR, in the chunk's own-tile order (the chunk's own kept
// points, grouped by row, input order within a row):
//   cnt    [F][n_chunks + 1][64] own points per row (k_feat_select turns them into row bases)
//   gidx   u16 per own-tile slot: the point's position in the chunk (frame-local index = chunk *
//          2048 + gidx), at idx_base(f) + chunk * 2048 + slot
//   gbits  per chunk three 2048-bit planes: planar candidate, UNRESOLVED, edge candidate
// A chunk cannot know a point's indexInRow j, only its rank in the window; but a stencil the
// window covers (5 row points on each side in the window) has 5 <= j < n_r - 5 necessarily, so its
// curvature decides the flags (frameFeature.cpp:84-107).  Every other own point of a row in range
// is marked unresolved: k_feat_select, which has the whole frame's counts, gives it curvature 0
// when j < 5 or j >= n_r - 5 (:85; always a planar candidate) and evaluates the rest -- open
// stencils, rare for azimuth-ordered scans -- through the chunk-major index, the same taps in the
// same order.  Every write of k_feat_chunk is a whole, aligned, contiguous run (no per-row
// scatter); the greedy of k_feat_select walks each row as its sequence of (chunk, row) segments.
#include "feat_common.hpp"

namespace ssf {

// LDS layouts of k_feat_chunk without write bank conflicts (ds_write_*: bank = (a / 4) mod 32,
// two 32-lane groups).  An azimuth-ordered scan puts one row per lane in every step, so a step's
// own-tile slots are p = seg(row) + q with seg spaced by the rows' own counts (32 for a full
// 2048-point chunk of a 64-beam scan): u16 slots 64 B apart (16-way), flag bytes 32 B apart
// (8-way).  XOR-swizzling bits 2..5 (idl) / 2..4 (flags) with the slot's row-size bits spreads
// them over every bank (2-way for the u16s: free for a store) and keeps 4-slot groups (8 B of
// idl) intact for the copy-out.  The f32 tile is padded by one float after every row run
// instead (runs of 44 floats: 12r mod 32 -> 45r mod 32), since its readers are 16-B loads.
static_assert(kTileE >= kWin + kMaxRows, "k_feat_chunk's tile holds the window plus one pad per row");
SSF_DEV int idl_sw(int p) { return p ^ (((p >> 6) & 15) << 2); }
SSF_DEV int fll_sw(int p) { return p ^ (((p >> 7) & 7) << 2); }

// The chunk's outputs from LDS (k_feat_chunk): the u16 chunk positions in
// own-tile order as whole 8-byte runs (idl, swizzled by idl_sw), and the candidate / unresolved
// (/ edge) bit planes packed from the flag bytes (fll, swizzled by fll_sw).
template <bool kEdge>
SSF_DEV void feat_chunk_out(int tid, int f, int c, int n_chunks, const int64_t* __restrict__ frame_off,
                            int clen, int no, const uint16_t* idl, const uint8_t* fll,
                            uint16_t* __restrict__ gidx, uint64_t* __restrict__ gbits) {
    uint16_t* gi = gidx + idx_base(frame_off, f) + (int64_t)c * kBinChunk;   // 4 KiB aligned run
    for (int k = tid; 4 * k < clen; k += kCurvNT)             // 8-byte stores (4 slots)
        *reinterpret_cast<uint2*>(gi + 4 * k) = *reinterpret_cast<const uint2*>(idl + 4 * (k ^ ((k >> 4) & 15)));
    uint64_t* gb = gbits + ((int64_t)f * n_chunks + c) * (kFeatPlanes * kFeatWords);
    constexpr int kPl = kEdge ? 3 : 2;
    if (tid < kPl * kFeatWords) {
        const int pl = tid / kFeatWords, wi = tid - pl * kFeatWords;
        const int nbit = min(64, max(0, no - 64 * wi));
        uint64_t wv = 0;
        if (nbit > 0) {
            uint64_t b8[8];
            const int sw = (wi >> 1) & 7;                     // fll_sw of this word's 64 flags
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const uint64_t x = *reinterpret_cast<const uint64_t*>(fll + 8 * ((8 * wi + u) ^ (sw >> 1)));
                b8[u] = (sw & 1) ? ((x >> 32) | (x << 32)) : x;
            }
            wv = pack64(b8, pl);                              // bit pl of every flag byte
            if (nbit < 64) wv &= (1ull << nbit) - 1ull;
        }
        gb[pl * kFeatWords + wi] = wv;
    }
}

// One (frame, chunk) block of k_feat_chunk / k_feat_chunk_flagged (the work-group's LDS is
// declared here: one block at a time)
template <bool kDebug, bool kEdge>
SSF_DEV void feat_chunk_block(int64_t lb, const float* __restrict__ pts, int stride,
                                                    const int64_t* __restrict__ frame_off,
                                                    int n_frames, int n_rows, int n_chunks,
                                                    int row_start, int row_end, float plane_min,
                                                    float edge_min, const uint8_t* __restrict__ keep,
                                                    const RingTable* __restrict__ rtab,
                                                    int32_t* __restrict__ cnt,
                                                    uint16_t* __restrict__ gidx,
                                                    uint64_t* __restrict__ gbits,
                                                    float* __restrict__ curv_cm) {
    __shared__ __attribute__((aligned(16))) float sc[kTileE + 2 * kTilePad];   // x, then y, then z
    __shared__ __attribute__((aligned(16))) uint16_t meta[kTileE];   // own-tile slot | 0x8000: stencil
    // two LDS regions reused across phases (31 KiB in all: 5 work-groups per CU):
    //   A: the ring-id table (ids) -> u16 chunk position per own-tile slot (place, out)
    //   B: the per-row lane words (rank) -> the flag byte per own-tile slot (place, curvature, out)
    __shared__ __attribute__((aligned(16))) char regA[(kBinChunk + 4) * 2];
    __shared__ __attribute__((aligned(16))) char regB[kCurvNW * (kMaxRows + 1) * 8];
    static_assert(sizeof(regA) >= kRingCells * sizeof(RingCell) && sizeof(regB) >= kBinChunk, "LDS reuse");
    RingCell* rcell = reinterpret_cast<RingCell*>(regA);
    uint16_t* idl = reinterpret_cast<uint16_t*>(regA);
    auto gmask = reinterpret_cast<unsigned long long (*)[kMaxRows + 1]>(regB);
    uint8_t* fll = reinterpret_cast<uint8_t*>(regB);
    // per (wave, row): the wave's row points so far, packed {all : 16, halo-before : 16,
    // halo-before + own : 16} -- one word read and rewritten per step, no atomics
    __shared__ unsigned long long wrun[kCurvNW][kMaxRows + 1];
    // per (wave, row), in the rank space q of the wave's points of that row: tile slot base,
    // own-tile slot base, the ranks whose 11 taps the window holds
    __shared__ int4 wrec[kCurvNW][kMaxRows];
    __shared__ int ntot, nown;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: step masks in SGPRs
    const int f = (int)(lb / n_chunks), c = (int)(lb - (int64_t)f * n_chunks);
    const int64_t fb = frame_off[f], e = frame_off[f + 1];
    const int64_t s = fb + (int64_t)c * kBinChunk;
    if (s >= e) return;                                       // uniform
    const int64_t t = min(e, s + (int64_t)kBinChunk);
    const int64_t ws = max(fb, s - (int64_t)kCurvHalo), we = min(e, t + (int64_t)kCurvHalo);
    const int L = (int)(we - ws), hb = (int)(s - ws), he = (int)(t - ws);   // own: [hb, he)
    const int qlen = ((L + kCurvNW - 1) / kCurvNW + 63) / 64 * 64;
    const int q0 = w * qlen, q1 = min(L, q0 + qlen);
    int idr[kWinQ];
    float px[kWinQ], py[kWinQ], pz[kWinQ];
    const float* pw = pts + ws * stride;
    // every point load first (clamped, unconditional), in flight across the LDS set-up and its
    // barrier -- the ring table's load no longer goes ahead of them
#pragma unroll
    for (int st = 0; st < kWinQ; ++st) {
        const float* pp = pw + (uint32_t)(min(q0 + lane + 64 * st, L - 1) * stride);
        px[st] = pp[0]; py[st] = pp[1]; pz[st] = pp[2];
    }
    uint8_t kp[kWinQ];
    if (keep) {
#pragma unroll
        for (int st = 0; st < kWinQ; ++st) kp[st] = keep[ws + min(q0 + lane + 64 * st, L - 1)];
    }
    if (tid < kMaxRows) {
#pragma unroll
        for (int k = 0; k < kCurvNW; ++k) { wrun[k][tid] = 0ull; gmask[k][tid] = 0ull; }
    }
    if (tid < kCurvNW) { wrun[tid][kMaxRows] = 0ull; gmask[tid][kMaxRows] = 0ull; }
    for (int k = tid; k < kRingCells; k += kCurvNT) rcell[k] = rtab->cell[k];
    const float r0 = rtab->r0, rinv = rtab->inv;
    __syncthreads();
#pragma unroll
    for (int st = 0; st < kWinQ; ++st) {                      // frameFeature.cpp:57-73
        const bool in = q0 + lane + 64 * st < q1 && (!keep || kp[st]);
        const int id = ring_id_table(px[st], py[st], pz[st], r0, rinv, rcell, rtab);   // every lane: no branch
        idr[st] = in ? id : -1;
    }
    // rank among same-row points (the k_bin_curv ranking: per-row lane words, waves in order).
    // Every lane of a row computes the same new counter word and writes it (and clears the lane
    // word): the wave's LDS instructions complete in order, so all reads of the step precede
    // these writes -- no leader branch.  The halo-before / own lanes of a step are uniform masks.
#pragma unroll
    for (int st = 0; st < kWinQ; ++st) {
        const int id = idr[st];
        const int rs = id >= 0 ? id : kMaxRows;
        unsigned long long* gm = &gmask[w][rs];
        __hip_atomic_fetch_or(gm, 1ull << lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const uint64_t m = __hip_atomic_load(gm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const uint64_t old = wrun[w][rs];
        const int s0 = q0 + 64 * st;                          // uniform
        const int hbl = __builtin_amdgcn_readfirstlane(min(64, max(0, hb - s0)));   // SGPRs
        const int hel = __builtin_amdgcn_readfirstlane(min(64, max(0, he - s0)));
        const int rin = __popcll(m & lanemask_lt());
        const uint64_t pm = (uint64_t)__popcll(m);
        const uint64_t hm = hbl >= 64 ? ~0ull : ((1ull << hbl) - 1ull);   // lanes before the chunk
        const uint64_t om = hel >= 64 ? ~0ull : ((1ull << hel) - 1ull);   // lanes before its end
        const uint64_t inc = pm + ((uint64_t)__popcll(m & hm) << 16) + ((uint64_t)__popcll(m & om) << 32);
        wrun[w][rs] = old + inc;
        __hip_atomic_store(gm, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        idr[st] = (id & 0xff) | (((int)(old & 0xffffu) + rin) << 8);
    }
    __syncthreads();
    if (tid < 64) {                                           // rows on the lanes of wave 0
        const int r = tid;
        int tot = 0, nbr = 0, obr = 0;
        int pwk[kCurvNW];
        if (r < n_rows) {
#pragma unroll
            for (int k = 0; k < kCurvNW; ++k) {
                const uint64_t v = wrun[k][r];
                pwk[k] = tot;                                 // the wave's first position in the run
                tot += (int)(v & 0xffffu);
                nbr += (int)((v >> 16) & 0xffffu);
                obr += (int)((v >> 32) & 0xffffu);
            }
        }
        const int own = r < n_rows ? obr - nbr : 0;
        int incl = tot, oincl = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o, 64), yo = __shfl_up(oincl, o, 64);
            if (r >= o) { incl += y; oincl += yo; }
        }
        cnt[((int64_t)f * (n_chunks + 1) + c) * kMaxRows + r] = own;
        if (r < n_rows) {
            const int run0 = incl - tot, seg0 = oincl - own;
#pragma unroll
            for (int k = 0; k < kCurvNW; ++k)
                wrec[k][r] = make_int4(run0 + r + pwk[k], seg0 + pwk[k] - nbr, 5 - pwk[k], tot - 5 - pwk[k]);
            meta[run0 + r + tot] = 0;                         // the row run's pad entry: no stencil
        }
        if (r == 63) { ntot = incl + n_rows; nown = oincl; }  // tile entries incl. one pad per row
    }
    __syncthreads();
    const int nt = ntot;
    const int64_t cm = fb + (int64_t)c * kBinChunk;           // chunk-major base (curvature)
    // ---- place: tile slot of every window point, own-tile slot + position of every own point
    int loc[kWinQ];
#pragma unroll
    for (int st = 0; st < kWinQ; ++st) {
        const int id = (int)(int8_t)(idr[st] & 0xff);
        loc[st] = kTileE;                                     // no point: the pad slot
        if (id >= 0) {
            const int q = idr[st] >> 8;
            const int4 rw = wrec[w][id];
            const int k = rw.x + q;
            const int wp = q0 + lane + 64 * st;
            const bool own = wp >= hb && wp < he;
            const bool row_in = id >= row_start && id < n_rows - row_end;
            const bool covered = q >= rw.z && q < rw.w;
            uint16_t mk = 0;
            if (own) {
                const int p = rw.y + q;
                idl[idl_sw(p)] = (uint16_t)(wp - hb);
                if (row_in && covered) {
                    mk = (uint16_t)(p | 0x8000);
                } else {
                    fll[fll_sw(p)] = row_in ? kFlU : (uint8_t)0;
                    if (kDebug && curv_cm) curv_cm[cm + p] = 0.0f;
                }
            }
            meta[k] = mk;
            sc[kTilePad + k] = px[st];
            loc[st] = k;
        }
    }
    __syncthreads();
    // ---- curvature of this thread's kCE tile entries, one coordinate at a time (k_bin_curv)
    const int k0 = kCE * tid;
    float v[kCE];
    auto coord = [&](float (&d)[kCE]) {
        float h[kCE + 16];
#pragma unroll
        for (int k = 0; k < (kCE + 16) / 4; ++k) {
            const float4 x4 = *reinterpret_cast<const float4*>(sc + k0 + 4 * k);
            h[4 * k] = x4.x; h[4 * k + 1] = x4.y; h[4 * k + 2] = x4.z; h[4 * k + 3] = x4.w;
        }
#pragma unroll
        for (int i = 0; i < kCE; ++i) d[i] = tap11(h + 3 + i);
    };
    {
        // ((dX dX + dY dY) + dZ dZ), each product rounded: the square of one coordinate's sum is
        // kept, not the sum itself (one kCE array live instead of two)
        float d0[kCE];
        coord(d0);
#pragma unroll
        for (int i = 0; i < kCE; ++i) v[i] = d0[i] * d0[i];
        __syncthreads();
#pragma unroll
        for (int st = 0; st < kWinQ; ++st) sc[kTilePad + loc[st]] = py[st];
        __syncthreads();
        coord(d0);
#pragma unroll
        for (int i = 0; i < kCE; ++i) v[i] = v[i] + d0[i] * d0[i];
        __syncthreads();
#pragma unroll
        for (int st = 0; st < kWinQ; ++st) sc[kTilePad + loc[st]] = pz[st];
        __syncthreads();
        coord(d0);
#pragma unroll
        for (int i = 0; i < kCE; ++i) v[i] = v[i] + d0[i] * d0[i];
    }
    uint16_t mt[kCE];
#pragma unroll
    for (int i = 0; i < kCE; i += 4) {                        // k0 + kCE <= kTileE: 8-byte reads
        const uint2 m2 = *reinterpret_cast<const uint2*>(meta + k0 + i);
        mt[i] = (uint16_t)(m2.x & 0xffffu); mt[i + 1] = (uint16_t)(m2.x >> 16);
        mt[i + 2] = (uint16_t)(m2.y & 0xffffu); mt[i + 3] = (uint16_t)(m2.y >> 16);
    }
#pragma unroll
    for (int i = 0; i < kCE; ++i) {
        if (k0 + i < nt && (mt[i] & 0x8000)) {
            const int p = mt[i] & 0x7fff;
            const uint8_t fl = cand_flags(true, true, v[i], plane_min, kEdge, edge_min);
            fll[fll_sw(p)] = (uint8_t)((fl & 1) ? kFlP : 0) | (uint8_t)((fl & 2) ? kFlE : 0);
            if (kDebug && curv_cm) curv_cm[cm + p] = v[i];
        }
    }
    __syncthreads();
    // ---- out: the chunk's own-tile slots, whole aligned runs
    feat_chunk_out<kEdge>(tid, f, c, n_chunks, frame_off, (int)(t - s), nown, idl, fll, gidx, gbits);
}

#define SSF_FC_ARGS pts, stride, frame_off, n_frames, n_rows, n_chunks, row_start, row_end, plane_min, \
                    edge_min, keep, rtab, cnt, gidx, gbits, curv_cm
#define SSF_FC_PARAMS const float* __restrict__ pts, int stride, const int64_t* __restrict__ frame_off, \
    int n_frames, int n_rows, int n_chunks, int row_start, int row_end, float plane_min,              \
    float edge_min, const uint8_t* __restrict__ keep, const RingTable* __restrict__ rtab,             \
    int32_t* __restrict__ cnt, uint16_t* __restrict__ gidx, uint64_t* __restrict__ gbits,            \
    float* __restrict__ curv_cm
// every (frame, chunk) block, one per work-group (XCD-aware: each XCD walks a contiguous range, so
// a window's halo was just read into its own L2)
template <bool kDebug, bool kEdge>
__global__ __launch_bounds__(kCurvNT, SSF_FEAT_WAVES) void k_feat_chunk(SSF_FC_PARAMS) {
    const int64_t nblk = (int64_t)n_chunks * n_frames;
    const int64_t q8 = (nblk + 7) / 8;
    const int64_t lb = (int64_t)(blockIdx.x % 8) * q8 + blockIdx.x / 8;
    if (lb >= nblk) return;
    feat_chunk_block<kDebug, kEdge>(lb, SSF_FC_ARGS);
}

// after k_feat_wave_reg / k_feat_wave_run: only the blocks they flagged.  A work-group reads the flags of 16
// consecutive blocks in one 16-byte load and does the flagged ones in turn, so a launch of
// regular frames is nblk / 16 work-groups that return at once (one work-group per block cost
// ~9 us to drain for 15 k blocks)
constexpr int kFlagGroup = 16;
template <bool kDebug, bool kEdge>
__global__ __launch_bounds__(kCurvNT, SSF_FEAT_WAVES) void k_feat_chunk_flagged(SSF_FC_PARAMS,
                                                                             const uint8_t* __restrict__ irregular) {
    const int64_t nblk = (int64_t)n_chunks * n_frames;
    const int64_t b0 = (int64_t)blockIdx.x * kFlagGroup;
    const uint4 fw = *reinterpret_cast<const uint4*>(irregular + b0);   // feat_irr_bytes: 16-B padded
    uint32_t m = 0;
    const uint32_t wd[4] = {fw.x, fw.y, fw.z, fw.w};
#pragma unroll
    for (int k = 0; k < kFlagGroup; ++k) m |= (uint32_t)(((wd[k >> 2] >> (8 * (k & 3))) & 0xffu) == kIrrGeneral) << k;
    while (m) {                                               // uniform
        const int k = __builtin_ctz(m);
        m &= m - 1u;
        if (b0 + k >= nblk) break;
        feat_chunk_block<kDebug, kEdge>(b0 + k, SSF_FC_ARGS);
        __syncthreads();                                      // the block's LDS readers are done
    }
}
#undef SSF_FC_ARGS
#undef SSF_FC_PARAMS

void launch_feat_chunk(const FeatLaunch& a, const FeatScratch& fs) {
    const FeatFrames& in = a.in;
    const ssf_config& cfg = a.cfg;
    const RingTable* rt = reinterpret_cast<const RingTable*>(fs.rtab);
    const int64_t nblk = (int64_t)a.n_chunks * a.n_frames;
    kmark(a.s, fs.irr ? "k_feat_chunk_flagged" : "k_feat_chunk");
    dispatch_de(a.dbg, a.edge, [&](auto D, auto E) {
        constexpr bool kD = decltype(D)::value, kE = decltype(E)::value;
        if (fs.irr)
            hipLaunchKernelGGL((k_feat_chunk_flagged<kD, kE>), dim3((unsigned)((nblk + kFlagGroup - 1) / kFlagGroup)),
                               dim3(kCurvNT), 0, a.s, in.pts, in.stride, in.frame_off, a.n_frames, cfg.n_rows,
                               a.n_chunks, cfg.row_start, cfg.row_end, cfg.plane_min, a.es.min_curv, in.keep, rt,
                               fs.cnt, fs.gidx, fs.gbits, fs.curv_cm, fs.irr);
        else
            hipLaunchKernelGGL((k_feat_chunk<kD, kE>), dim3((unsigned)((nblk + 7) / 8 * 8)), dim3(kCurvNT), 0,
                               a.s, in.pts, in.stride, in.frame_off, a.n_frames, cfg.n_rows, a.n_chunks,
                               cfg.row_start, cfg.row_end, cfg.plane_min, a.es.min_curv, in.keep, rt, fs.cnt,
                               fs.gidx, fs.gbits, fs.curv_cm);
    });
}

}  // namespace ssf
