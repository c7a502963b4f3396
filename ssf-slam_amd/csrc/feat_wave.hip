// feat_wave.hip -- the one-wave-per-chunk kernels of the single-read feature stage.  Each writes
// what k_feat_chunk (feat_chunk.hip) would for the chunks whose layout it knows, and flags the
// others kIrrGeneral for the kernels launched after it:
//   k_feat_wave_reg  regular windows: an azimuth-ordered 64-beam scan, one row per lane
//   k_feat_wave_run  rows as runs of consecutive inputs: channel-major sweeps, 16 beams, masks
#include "feat_common.hpp"

#include <cmath>

namespace ssf {

// k_feat_wave_reg: k_feat_chunk's outputs for REGULAR windows with ONE WAVE per chunk.
// Regular is the common layout of a 64-beam scan in azimuth order (the reference's driver order;
// the bench's synthetic scans): the window is whole columns of 64 points, each column holds every
// row once, and lane l of every column is the same row.  Then a row's points in the window are
// one lane's column sequence -- rank = column, the own-tile slot is row x own columns + (column -
// first own column), and the 11 taps of a stencil are that lane's columns c - 5 .. c + 5 -- so
// there is no ranking, no placement and no row-grouped tile, a chunk's whole stencil work needs
// no other wave, and a work-group is kCurvNW independent chunks with no barrier at all.  A window
// that is not regular (masked points, a ragged frame end, a point without a row, another order)
// is flagged for the kernels launched after this one.  Each wave loads the ring table into registers (lane l: cells 4l .. 4l + 3,
// rlo / rhi of row l; a lookup is a lane permute), then the chunk's 32 own columns and the 5 on
// each side (42 column loads of 768 B, streamed in blocks of kWB own columns, see stream below),
// checks regularity, evaluates every covered stencil from registers and builds the
// candidate / unresolved / edge bits of its own points as per-lane
// masks (bit i = own column i), OR-ed into the chunk's bit planes in the wave's LDS words
// (own-tile slot p = row x own columns + i) and stored as whole words.  The window's outermost
// columns (one each side of a full 6-column halo) are not loaded: no stencil of an own point
// reaches them, and they cannot change whether one is covered (a covered own point's 5 row
// neighbours on each side lie in the checked columns, which hold its row exactly once each), so
// the outputs are those of k_feat_chunk on every window this kernel calls regular.
constexpr int kWaveOwn = kBinChunk / 64;         // own columns of a full chunk (32)
constexpr int kWaveCols = kWaveOwn + 10;         // columns a wave loads
constexpr int kWB = SSF_FEAT_WAVE_BLOCK;
static_assert(kWaveOwn % kWB == 0, "whole blocks");
static_assert(kRingCells == 4 * 64 && kWaveOwn <= 32 && kCurvHalo >= 5 * 64,
              "ring table: 4 cells per lane; own-column masks are 32 bits; 5 halo columns");

// the table's cell ci from the lanes' registers (every lane must be active)
SSF_DEV RingCell cell_from_lanes(int ci, const float (&thr)[4], const int (&ids)[4]) {
    const int src = ci >> 2, q = ci & 3;
    float t4[4];
    int i4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { t4[k] = __shfl(thr[k], src, 64); i4[k] = __shfl(ids[k], src, 64); }
    RingCell rc;
    rc.thr = q == 0 ? t4[0] : q == 1 ? t4[1] : q == 2 ? t4[2] : t4[3];
    rc.ids = q == 0 ? i4[0] : q == 1 ? i4[1] : q == 2 ? i4[2] : i4[3];
    return rc;
}

template <bool kDebug, bool kEdge>
__global__ __launch_bounds__(kCurvNT, (kDebug || kEdge) ? 3 : SSF_FEAT_WAVE_WAVES) void k_feat_wave_reg(
    const float* __restrict__ pts, int stride, const int64_t* __restrict__ frame_off, int n_frames,
    int n_rows, int n_chunks, int row_start, int row_end, float plane_min, float edge_min,
    const RingTable* __restrict__ rtab, int32_t* __restrict__ cnt, uint16_t* __restrict__ gidx,
    uint64_t* __restrict__ gbits, float* __restrict__ curv_cm, uint8_t* __restrict__ irregular,
    uint8_t* __restrict__ lanemap) {
    __shared__ unsigned long long wpl[kCurvNW][kFeatPlanes * kFeatWords];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t nblk = (int64_t)n_chunks * n_frames;
    const int64_t nwg = (nblk + kCurvNW - 1) / kCurvNW;       // XCD-aware logical work-group
    const int64_t q8 = (nwg + 7) / 8;
    const int64_t lw = (int64_t)(blockIdx.x % 8) * q8 + blockIdx.x / 8;
    const int64_t lb = lw * kCurvNW + w;                      // this wave's (frame, chunk)
    if (lw >= nwg || lb >= nblk) return;                      // uniform per wave (no barrier below)
    const int f = (int)(lb / n_chunks), c = (int)(lb - (int64_t)f * n_chunks);
    const int64_t fb = frame_off[f], e = frame_off[f + 1];
    const int64_t s = fb + (int64_t)c * kBinChunk;
    if (s >= e) {                                             // uniform: no chunk here at all
        if (lane == 0) irregular[lb] = 0;
        return;
    }
    const int64_t t = min(e, s + (int64_t)kBinChunk);
    const int64_t ws = max(fb, s - (int64_t)kCurvHalo), we = min(e, t + (int64_t)kCurvHalo);
    const int L = (int)(we - ws), hb = (int)(s - ws), he = (int)(t - ws);
    if (((L | hb | he) & 63) != 0) {                          // uniform: not whole columns
        if (lane == 0) irregular[lb] = 1;
        return;
    }
    // the table first: its loads are then the first to complete
    const float4 th4 = *reinterpret_cast<const float4*>(&rtab->cell[4 * lane]);          // cells 4l, 4l + 1
    const float4 th4b = *reinterpret_cast<const float4*>(&rtab->cell[4 * lane + 2]);     // 4l + 2, 4l + 3
    const float rlo_l = rtab->rlo[lane], rhi_l = rtab->rhi[lane];
    const float r0 = rtab->r0, rinv = rtab->inv;
    const bool dchain = rtab->chain == kRingChainDouble;      // uniform (a scalar load)
    const int ncols = L >> 6, c_hb = hb >> 6, oc = (he - hb) >> 6;
    const int j0 = c_hb - 5;                                  // window column of register k = 0
    const int klo = max(0, -j0), khi = min(kWaveCols, ncols - j0);   // registers holding real columns
    // x and y of a column side by side (the dwordx3 load's first two registers): the stencils of
    // x and y run as packed f32 pairs (v_pk_add_f32 / v_pk_mul_f32: two IEEE operations with
    // the rounding of two scalar ones, the reference's order kept), z alone
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 XY[kWaveCols];
    float Z[kWaveCols];
    // a column's base is uniform (SGPRs), the lane's byte offset one 32-bit VGPR for every column
    const uint32_t lob = (uint32_t)(lane * stride) * 4u;
    const char* wbase = reinterpret_cast<const char*>(pts + ws * stride);
    const uint32_t colb = 256u * (uint32_t)stride;            // bytes per column (< 2^31: checked at launch)
    auto load_col = [&](int k) {
        const uint32_t o = (uint32_t)min(max(j0 + k, 0), ncols - 1) * colb + lob;
        const float3 p3 = *reinterpret_cast<const float3*>(wbase + o);
        XY[k] = f2{p3.x, p3.y}; Z[k] = p3.z;
    };
    wpl[w][lane] = 0ull;                                      // the wave's plane words
    if (lane < kFeatPlanes * kFeatWords - 64) wpl[w][64 + lane] = 0ull;
    const float thr[4] = {th4.x, th4.z, th4b.x, th4b.z};
    const int ids[4] = {__float_as_int(th4.y), __float_as_int(th4.w), __float_as_int(th4b.y), __float_as_int(th4b.w)};
    int mine = -1, row = 0;
    float rlo = 0.f, rhi = 0.f;
    unsigned long long rows = 0ull;
    bool row_in = false;
    uint64_t inb = 0, need = 0;
    uint32_t mp = 0, mu = 0, me = 0;
    const int64_t cm = fb + (int64_t)c * kBinChunk;           // chunk-major base (curvature)
    uint16_t* gi = gidx + idx_base(frame_off, f) + (int64_t)c * kBinChunk;
    // every real column's point inside the row's ratio interval, clear of both ends by the row's
    // margin 1e-6 max(1, |rlo|, |rhi|) -- at least ring_id_table's per-point 1e-6 max(1, |ra|)
    // for any ra inside, so the fast ratio's row is the exact one -- folded into the
    // bounds once per lane (rlo / rhi below): per column one rsq, one multiply, four compares
    auto check_col = [&](int k) {
        const f2 q2 = XY[k] * XY[k];
        const float r2 = q2.x + q2.y;
        const float ra = Z[k] * __builtin_amdgcn_rsqf(r2);
        const bool in = ra >= rlo && ra < rhi && r2 > 1e-30f && r2 < 1e30f;
        inb |= (uint64_t)in << k;
        need |= (uint64_t)(k >= klo && k < khi) << k;         // uniform
    };
    // The columns stream in blocks of kWB own columns: the first block's window (kWB + 10
    // columns), then each block's loads issued before the previous block's stencils.  Even chunks
    // stream left to right, odd chunks right to left, so the 5 columns two neighbouring chunks
    // share are loaded by both at the same end of their streams, close in time (an L2 hit for the
    // later one: streaming both ways from the left, the right neighbour's copy had left the L2).
    constexpr int nb = kWaveOwn / kWB;
    auto stream = [&](auto rev) -> bool {
        constexpr bool R = decltype(rev)::value;
        constexpr int kf = R ? kWaveCols - 6 : 5;              // an own column of the first window
        constexpr int f0 = R ? kWB * (nb - 1) : 0;             // the first window [f0, f0 + kWB + 10)
        // that column first: a chunk whose first column is not one row per lane (any other layout,
        // e.g. channel-major CARLA sweeps) leaves before the other 41 columns are read
        load_col(kf);
        // the lane's row from that column (a clamped load is still a real column, and every real
        // column is checked below): ring_id_table's test with the cells from lane permutes (the
        // exact ratio's cell fetched for every lane, used where the fast one is near)
        {
            const float x = XY[kf].x, y = XY[kf].y, z = Z[kf];
            const float r2 = x * x + y * y;
            const float ra = z * __builtin_amdgcn_rsqf(r2);
            int ci = (int)((ra - r0) * rinv);
            ci = min(max(ci, 0), kRingCells - 1);
            const RingCell rc = cell_from_lanes(ci, thr, ids);
            const float m = 1e-6f * fmaxf(1.0f, fabsf(ra));
            const float tc = (ra - r0) * rinv, fr = tc - floorf(tc);
            const int near = (int)!(fabsf(ra - rc.thr) > m) | (int)!(fr > m * rinv) | (int)!(fr < 1.0f - m * rinv) |
                             (int)!(r2 > 1e-30f) | (int)!(r2 < 1e30f);
            // ring_id_exact's ratio: the float chain's z / sqrtf(r2), or the double chain's
            // double ratio (its cell from the float rounding, its threshold the cell's double)
            float rx;
            double dr = 0.0;
            if (dchain) { dr = (double)z / sqrt((double)r2); rx = (float)dr; }   // uniform
            else rx = z / sqrtf(r2);
            int cx = (int)((rx - r0) * rinv);
            cx = min(max(cx, 0), kRingCells - 1);
            const RingCell rcx = cell_from_lanes(cx, thr, ids);
            const int a = (int)(int8_t)(rc.ids & 0xff), b = (int)(int8_t)((rc.ids >> 8) & 0xff);
            const int ax = (int)(int8_t)(rcx.ids & 0xff), bx = (int)(int8_t)((rcx.ids >> 8) & 0xff);
            int idx = rx == rx ? (rx < rcx.thr ? ax : bx) : -1;
            if (dchain) idx = dr == dr ? (dr < rtab->dthr[cx] ? ax : bx) : -1;
            mine = near ? idx : (ra < rc.thr ? a : b);
        }
        row = mine & (kMaxRows - 1);
        {
            const float lo = __shfl(rlo_l, row, 64), hi = __shfl(rhi_l, row, 64);
            const float m = 1e-6f * fmaxf(1.0f, fmaxf(fabsf(lo), fabsf(hi)));
            rlo = lo + m;                                      // the check's bounds, margins in
            rhi = hi - m;
        }
        rows = 1ull << row;                                    // every row once per column
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) rows |= __shfl_xor(rows, o, 64);
        if (rows != ~0ull || !__all(mine >= 0 && mine < kMaxRows)) return false;   // uniform
        asm volatile("" ::: "memory");                         // no column load above the probe
#pragma unroll
        for (int k = f0; k < f0 + kWB + 10; ++k)
            if (k != kf) load_col(k);
        row_in = row >= row_start && row < n_rows - row_end;
#pragma unroll
        for (int k = f0; k < f0 + kWB + 10; ++k) check_col(k);
        // stencils of the own columns (window column c_hb + i, registers i .. i + 10), the flags
        // as bit i of per-lane masks: planar candidate, unresolved, edge candidate
#pragma unroll
        for (int bs = 0; bs < nb; ++bs) {
            const int bk = R ? nb - 1 - bs : bs;               // this block
            const int n0 = R ? kWB * (bk - 1) : kWB * (bk + 1) + 10;   // the next block's new columns
            if (bs + 1 < nb) {                                 // ... in flight
#pragma unroll
                for (int k = n0; k < n0 + kWB; ++k) load_col(k);
            }
#pragma unroll
            for (int i = kWB * bk; i < kWB * (bk + 1); ++i) { // no branch: columns past oc masked
                const int col = c_hb + i;
                const bool own = i < oc, covered = col >= 5 && col < ncols - 5;   // uniform
                f2 dxy = XY[i] + XY[i + 1];                   // tap11 of x and y (frameFeature.cpp:88-97)
#pragma unroll
                for (int k = 2; k < 11; ++k) dxy = (k == 5) ? dxy - f2{10.0f, 10.0f} * XY[i + 5] : dxy + XY[i + k];
                const float dz = tap11(Z + i);
                const f2 sq = dxy * dxy;
                float v = sq.x + sq.y;                        // ((dX dX + dY dY) + dZ dZ)
                v = v + dz * dz;
                const uint8_t cf = cand_flags(true, true, v, plane_min, kEdge, edge_min);
                const bool dec = own && row_in && covered;
                mp |= (uint32_t)(dec && (cf & 1)) << i;
                if (kEdge) me |= (uint32_t)(dec && (cf & 2)) << i;
                mu |= (uint32_t)(own && row_in && !covered) << i;
                if (kDebug && own) {                          // (an irregular chunk's are rewritten)
                    const int p = row * oc + i;
                    gi[p] = (uint16_t)(64 * i + lane);
                    if (curv_cm) curv_cm[cm + p] = dec ? v : 0.0f;
                }
            }
            // the block's stencils complete here, and no load moves across: 26 columns live, not 42
            asm volatile("" : "+v"(mp), "+v"(mu), "+v"(me), "+v"(inb) : : "memory");
            if (bs + 1 < nb) {
#pragma unroll
                for (int k = n0; k < n0 + kWB; ++k) check_col(k);
            }
        }
        return true;
    };
    const bool probed = (c & 1) ? stream(std::true_type{}) : stream(std::false_type{});   // uniform
    if (!probed) {                                            // not one row per lane: not regular
        if (lane == 0) irregular[lb] = kIrrGeneral;
        return;
    }
    const bool ok = mine >= 0 && mine < kMaxRows && (inb & need) == need && rows == ~0ull;
    if (!__all(ok)) {                                         // uniform: the general kernel's chunk
        if (lane == 0) irregular[lb] = 1;
        return;
    }
    // own-tile bits [row x oc, row x oc + oc) of each plane: at most two 64-bit words
    const int p0 = row * oc, wlo = p0 >> 6, sh = p0 & 63;
    const bool spill = sh + oc > 64;
    const uint32_t mk[kFeatPlanes] = {mp, mu, me};
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");    // the zeroed words before the ORs
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int pl = 0; pl < (kEdge ? 3 : 2); ++pl) {
        const uint64_t bm = mk[pl];
        if (bm) {
            __hip_atomic_fetch_or(&wpl[w][pl * kFeatWords + wlo], bm << sh, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_WORKGROUP);
            if (spill)
                __hip_atomic_fetch_or(&wpl[w][pl * kFeatWords + wlo + 1], bm >> (64 - sh), __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
    uint64_t* gb = gbits + ((int64_t)f * n_chunks + c) * (kFeatPlanes * kFeatWords);
    gb[lane] = __hip_atomic_load(&wpl[w][lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // planes 0, 1
    if (kEdge && lane < kFeatWords)
        gb[64 + lane] = __hip_atomic_load(&wpl[w][64 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    cnt[((int64_t)f * (n_chunks + 1) + c) * kMaxRows + lane] = oc;
    lanemap[lb * kMaxRows + row] = (uint8_t)lane;
    if (lane == 0) irregular[lb] = 0;
}

// k_feat_wave_run: the single-read feature stage for chunks whose rows come as RUNS of consecutive
// inputs -- the layout of the reference's own data: a CARLA sweep is stored channel-major (every
// return of a channel in azimuth order, then the next channel), with the no-return rays and the
// road dropped (launch/run_noSeg.launch:4 reads a road-removed set; Scenario_Traj.py:307-315),
// so rows are ragged and no column holds one point per row.  A stencil (frameFeature.cpp:84-107)
// whose 11 taps are 11 CONSECUTIVE INPUTS of one row is exactly the reference's, whatever the rest
// of the frame holds: consecutive inputs of a row are consecutive in its ring order (:73-80).  So
// ONE WAVE per 2048-point chunk streams the chunk as 64-lane registers (lane l of register k =
// input s - 5 + 54k + l: 54 centres and 5 halo lanes each side; coalesced 768-B loads) and
// evaluates the stencil ALONG THE LANES: each of the reference's left-to-right additions is one
// v_add_f32 whose first operand is the partial sum one lane down (DPP wave_shr:1, free inside the
// instruction), so centre i's sum arrives in lane i + 5 after 11 dependent operations per
// coordinate, with tap11's roundings in tap11's order (lane_tap11x3).  Row ids: the fast ratio
// against the current row's interval (as k_feat_wave_reg's check); a register wholly inside it is
// one row, any other takes the table lookup where the check fails.  A centre is covered when its
// 10 neighbours share its row (a 10-bit window of one ballot); an own point of a row in range that
// is not covered is unresolved (row end or open stencil: k_feat_select decides it).  The chunk's
// runs (and gaps of points in no row) are logged in input order as they start.  Own-tile slots
// need each row to be at most one run in the chunk (slot = the row's base + the point's offset in
// its run): the bit planes are built in input order and moved run by run to slot order (nothing
// moves for runs in ascending row order without gaps), and k_feat_select finds a point at its
// row's run start (u16, the chunk's first 64 index entries) + its offset.  A chunk with a row in
// two runs, or more than kRunMax runs, is left to k_feat_chunk (kIrrGeneral).
constexpr int kRunStep = 54;                     // new centres per 64-lane register
constexpr int kRunMax = 64;                      // runs (and gaps) logged per chunk
constexpr int kRunPF = SSF_FEAT_RUN_PF;

SSF_DEV float dpp_shr1(float v) {                // lane l <- lane l - 1 (lane 0 <- 0)
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x138, 0xf, 0xf, true));
}
SSF_DEV int dpp_shr1i(int v) { return __builtin_amdgcn_mov_dpp(v, 0x138, 0xf, 0xf, true); }

// tap11 along the lanes (see k_feat_wave_run), for x, y and z: lane L gets the sum of the centre in lane L - 5
// (valid for 10 <= L < 64).  P = x[l-1] + x[l]; three more `+ x` on the sum one lane down give
// x[l-4] + .. + x[l]; one lane down again `- 10 x[l]` is tap11's left half and centre; then five
// `+ x` on the sum one lane down add x[i+1] .. x[i+5] in order, the sum moving one lane each time.
// The three coordinates' chains step by step side by side: a DPP operand must not be read in the
// two cycles after the VALU op that wrote it, so one chain alone pays an s_nop per step.
SSF_DEV void lane_tap11x3(float x, float y, float z, float& dx, float& dy, float& dz) {
    float px = dpp_shr1(x) + x, py = dpp_shr1(y) + y, pz = dpp_shr1(z) + z;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        px = dpp_shr1(px) + x;
        py = dpp_shr1(py) + y;
        pz = dpp_shr1(pz) + z;
    }
    const float tx = 10.0f * x, ty = 10.0f * y, tz = 10.0f * z;
    px = dpp_shr1(px) - tx;
    py = dpp_shr1(py) - ty;
    pz = dpp_shr1(pz) - tz;
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        px = dpp_shr1(px) + x;
        py = dpp_shr1(py) + y;
        pz = dpp_shr1(pz) + z;
    }
    dx = px; dy = py; dz = pz;
}

// bits [a, a + n) of a bit array of nw words as the low bits (0 < n <= 64)
SSF_DEV uint64_t bits_at(const unsigned long long* W, int a, int n, int nw) {
    const int wi = a >> 6, sh = a & 63;
    uint64_t v = W[wi] >> sh;
    if (sh && wi + 1 < nw) v |= (uint64_t)W[wi + 1] << (64 - sh);
    return n >= 64 ? v : (v & ((1ull << n) - 1ull));
}

template <bool kDebug, bool kEdge>
__global__ __launch_bounds__(kCurvNT, kDebug ? 2 : SSF_FEAT_RUN_WAVES) void k_feat_wave_run(
    const float* __restrict__ pts, int stride, const int64_t* __restrict__ frame_off, int n_frames,
    int n_rows, int n_chunks, int row_start, int row_end, float plane_min, float edge_min,
    const uint8_t* __restrict__ keep, const RingTable* __restrict__ rtab, int32_t* __restrict__ cnt,
    uint16_t* __restrict__ gidx, uint64_t* __restrict__ gbits, float* __restrict__ curv_cm,
    uint8_t* __restrict__ irregular, int all) {
    constexpr int kPl = kEdge ? 3 : 2;
    constexpr int kPW = kFeatPlanes * kFeatWords;
    __shared__ unsigned long long wpos[kCurvNW][kPW];    // the flags in input order
    __shared__ unsigned long long wslt[kCurvNW][kPW];    // ... in own-tile slot order
    __shared__ int2 wrun[kCurvNW][kRunMax];              // (row or -1 for a gap, first own position)
    __shared__ int wlen[kCurvNW][kMaxRows];              // own points per row
    __shared__ int wnum[kCurvNW][kMaxRows];              // runs per row
    __shared__ int wst[kCurvNW][kMaxRows];               // run start per row
    __shared__ float wcv[kDebug ? kCurvNW : 1][kDebug ? kBinChunk : 1];   // debug: curvature, input order
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t nblk = (int64_t)n_chunks * n_frames;
    const int64_t nwg = (nblk + kCurvNW - 1) / kCurvNW;       // XCD-aware logical work-group
    const int64_t q8 = (nwg + 7) / 8;
    const int64_t lw = (int64_t)(blockIdx.x % 8) * q8 + blockIdx.x / 8;
    const int64_t lb = lw * kCurvNW + w;                      // this wave's (frame, chunk)
    if (lw >= nwg || lb >= nblk) return;                      // uniform per wave (no barrier below)
    if (!all && irregular[lb] != kIrrGeneral) return;          // uniform: a regular chunk, done
    const int f = (int)(lb / n_chunks), c = (int)(lb - (int64_t)f * n_chunks);
    const int64_t fb = frame_off[f], e = frame_off[f + 1];
    const int64_t s = fb + (int64_t)c * kBinChunk;
    if (s >= e) {                                             // uniform: no chunk here at all
        if (lane == 0) irregular[lb] = kIrrRegular;
        return;
    }
    const int nf = (int)(e - fb);
    const int len = (int)(min(e, s + (int64_t)kBinChunk) - s);
    const int nreg = (len + kRunStep - 1) / kRunStep;         // registers with own centres
    const int q0 = (int)(s - fb) - 5;                         // frame index of register 0, lane 0
    for (int k = lane; k < kPW; k += 64) { wpos[w][k] = 0ull; wslt[w][k] = 0ull; }
    wlen[w][lane] = 0;
    wnum[w][lane] = 0;
    const float r0 = rtab->r0, rinv = rtab->inv;
    const int rlim = n_rows - row_end;
    // the wave's current row and its fast-ratio bounds, margins in (k_feat_wave_reg's check)
    int g = -1;
    float glo = INFINITY, ghi = -INFINITY;
    bool gin_row = false;                                     // g is a row in range
    // a register's points: frame index q = q0 + 54 k + lane through a buffer resource over the
    // frame's points: a lane outside the frame (q < 0 wraps) reads zeros from the range check and
    // is marked by INF (lanes [lo, hi) of the register are in the frame), so no clamp, no 64-bit
    // address per load: one add per register
    typedef int i3v __attribute__((ext_vector_type(3)));
    const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(pts + fb * stride), (short)0, nf * stride * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t*>(keep ? keep + fb : keep), (short)0, keep ? nf : 0, 0x00020000);
    const uint32_t sb = (uint32_t)stride * 4u;
    const uint32_t voff0 = (uint32_t)(q0 + lane) * sb, vstep = (uint32_t)kRunStep * sb;
    auto load_reg = [&](int k, float& x, float& y, float& z, uint32_t& kp) {
        const i3v v = __builtin_amdgcn_raw_buffer_load_b96(prs, voff0 + (uint32_t)k * vstep, 0, 0);
        x = __int_as_float(v.x); y = __int_as_float(v.y); z = __int_as_float(v.z);
        kp = keep ? (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(krs, (uint32_t)(q0 + lane + kRunStep * k), 0, 0) : 1u;
    };
    auto lane_range = [](int lo, int hi) -> uint64_t {        // lanes [lo, hi) as a mask (0 <= lo, hi <= 64)
        if (hi <= lo) return 0ull;
        const uint64_t up = hi >= 64 ? ~0ull : ((1ull << hi) - 1ull);
        return up & (~0ull << lo);
    };
    int nrun = 0;
    // the flag masks of register k (bits 0 .. 53: own positions 54 k .. 54 k + 53) go to lane k
    // of these VGPRs (v_writelane: no SALU, no LDS), and become the input-order words after the
    // loop.  The scalar unit is the one all 32 waves of a CU share: the steady state below keeps
    // it to a few instructions per register (SQ counters, r5e: 2.8 k SALU per chunk saturated it).
    uint32_t vPl = 0, vPh = 0, vUl = 0, vUh = 0, vEl = 0, vEh = 0;
    auto wl = [](uint32_t& dst, uint32_t val, int k) {        // lane k of dst <- val (uniform)
        asm("v_writelane_b32 %0, %1, %2" : "+v"(dst) : "s"(val), "{m0}"(k));   // lane select in m0
    };
    auto put = [&](int k, uint64_t mP, uint64_t mE) {
        wl(vPl, (uint32_t)mP, k);
        wl(vPh, (uint32_t)(mP >> 32), k);
        if (kEdge) {
            wl(vEl, (uint32_t)mE, k);
            wl(vEh, (uint32_t)(mE >> 32), k);
        }
    };
    // registers 1 .. kint: every lane in the frame, 54 own centres, no keep mask ("interior")
    const int kint = keep ? 0 : min((nf - 64 - q0) / kRunStep, len / kRunStep - 1);
    // one register's work (k: register, c*: its points); false when the chunk has too many runs
    auto reg = [&](int k, float cx, float cy, float cz, uint32_t ck) -> bool {
        const float r2 = cx * cx + cy * cy;
        const float ra = cz * __builtin_amdgcn_rsqf(r2);
        // (no upper bound on r2 needed: r2 = +inf gives ra = 0 = the exact z / sqrtf(inf); the
        // lower one keeps zero and denormal r2 off the fast path)
        const uint64_t INR = __builtin_amdgcn_ballot_w64(ra >= glo) & __builtin_amdgcn_ballot_w64(ra < ghi) &
                             __builtin_amdgcn_ballot_w64(r2 > 1e-30f);
        if (k >= 1 && k <= kint && INR == ~0ull) {           // uniform: an interior register, all row g
            float dx, dy, dz;
            lane_tap11x3(cx, cy, cz, dx, dy, dz);
            float v = dx * dx + dy * dy;                      // ((dX dX + dY dY) + dZ dZ)
            v = v + dz * dz;
            const uint64_t R = gin_row ? ~0x3FFull : 0ull;    // own, row in range, covered
            const uint64_t mP = (R & __builtin_amdgcn_ballot_w64(v < plane_min)) >> 10;
            const uint64_t mE = kEdge ? ((R & __builtin_amdgcn_ballot_w64(v > edge_min)) >> 10) : 0ull;
            put(k, mP, mE);                                   // nothing unresolved (lanes k of vU stay 0)
            if (kDebug && lane >= 10) wcv[kDebug ? w : 0][kRunStep * k + lane - 10] = gin_row ? v : 0.0f;
            return true;
        }
        const int q = q0 + kRunStep * k;                      // frame index of lane 0 (uniform)
        const uint64_t INF = lane_range(max(0, -q), min(64, nf - q));
        const uint64_t OK = keep ? (INF & __builtin_amdgcn_ballot_w64(ck != 0u)) : INF;
        const uint64_t IN = OK & INR;
        const bool uni = IN == ~0ull;                         // the whole register is row g
        int id = g;
        if (!uni) {
            const bool in = (IN >> lane) & 1ull, ok = (OK >> lane) & 1ull;
            if (!in) id = ok ? ring_id_table(cx, cy, cz, r0, rinv, rtab->cell, rtab) : -1;
            const int last = __builtin_amdgcn_readlane(id, 63);
            if (last >= 0 && last != g) {                     // uniform: follow the last lane's row
                g = last;
                const float lo = rtab->rlo[g], hi = rtab->rhi[g];
                const float m = 1e-6f * fmaxf(1.0f, fmaxf(fabsf(lo), fabsf(hi)));
                glo = lo + m;
                ghi = hi - m;
                gin_row = g >= row_start && g < rlim;
            }
        }
        float dx, dy, dz;
        lane_tap11x3(cx, cy, cz, dx, dy, dz);
        float v = dx * dx + dy * dy;                          // ((dX dX + dY dY) + dZ dZ)
        v = v + dz * dz;
        // lane L >= 10: the centre in lane L - 5, own position a0 + L - 10
        const int a0 = kRunStep * k;
        const int nown = min(kRunStep, len - a0);             // >= 1
        const uint64_t OWN = lane_range(10, 10 + nown);
        uint64_t COV, ROWIN;
        if (uni) {                                            // from the wave's row g (SGPRs)
            COV = ~0ull;
            ROWIN = gin_row ? ~0ull : 0ull;
        } else {
            const int idp = dpp_shr1i(id);
            const uint64_t E = __builtin_amdgcn_ballot_w64(id >= 0) & __builtin_amdgcn_ballot_w64(id == idp);
            const uint64_t sh = E >> max(lane - 9, 0);       // inputs l - 1, l one row: bit l
            COV = __builtin_amdgcn_ballot_w64(lane >= 10 && (sh & 0x3FFull) == 0x3FFull);
            const int idc = __shfl(id, max(lane - 5, 0), 64);
            ROWIN = __builtin_amdgcn_ballot_w64(idc >= row_start) & __builtin_amdgcn_ballot_w64(idc < rlim);
        }
        const uint64_t DEC = OWN & ROWIN & COV;
        const uint64_t mP = (DEC & __builtin_amdgcn_ballot_w64(v < plane_min)) >> 10;   // cand_flags
        const uint64_t mU = (OWN & ROWIN & ~COV) >> 10;
        const uint64_t mE = kEdge ? ((DEC & __builtin_amdgcn_ballot_w64(v > edge_min)) >> 10) : 0ull;
        put(k, mP, mE);
        wl(vUl, (uint32_t)mU, k);
        wl(vUh, (uint32_t)(mU >> 32), k);
        if (kDebug && lane >= 10 && lane < 10 + nown) wcv[kDebug ? w : 0][a0 + lane - 10] = ((DEC >> lane) & 1ull) ? v : 0.0f;
        // the runs starting here: an own centre whose input before it is another row (or none)
        uint64_t RS;
        if (uni) RS = k == 0 ? (1ull << 5) : 0ull;
        else {
            const int idm = dpp_shr1i(id);
            RS = lane_range(5, 5 + nown) & (__builtin_amdgcn_ballot_w64(id != idm) | (k == 0 ? (1ull << 5) : 0ull));
        }
        while (RS) {                                          // uniform (SGPRs), in input order
            const int i = (int)__builtin_ctzll(RS);
            RS &= RS - 1ull;
            const int r = __builtin_amdgcn_readlane(id, i);
            if (nrun < kRunMax && lane == 0) wrun[w][nrun] = make_int2(r, a0 + i - 5);
            ++nrun;
        }
        return nrun <= kRunMax;
    };
    // SSF_FEAT_RUN_PF registers in flight per wave: a register is reloaded with the one
    // SSF_FEAT_RUN_PF ahead as soon as its points are taken (reloading after its use, in place,
    // measured slower: 0.101 against 0.099 ms, r5j)
    float X[kRunPF], Y[kRunPF], Z[kRunPF];
    uint32_t KP[kRunPF];
#pragma unroll
    for (int j = 0; j < kRunPF; ++j) load_reg(j, X[j], Y[j], Z[j], KP[j]);
    bool go = true;
    for (int k0 = 0; k0 < nreg && go; k0 += kRunPF) {        // uniform
#pragma unroll
        for (int j = 0; j < kRunPF; ++j) {
            if (go && k0 + j < nreg) {                        // uniform
                const float cx = X[j], cy = Y[j], cz = Z[j];
                const uint32_t ck = KP[j];
                load_reg(k0 + j + kRunPF, X[j], Y[j], Z[j], KP[j]);
                go = reg(k0 + j, cx, cy, cz, ck);
            }
        }
    }
    // the input-order words: lane t < 32 word t of the candidate plane, lane 32 + t of the
    // unresolved one (the edge plane next), each from the 1 .. 3 registers overlapping its bits
    {
        auto word = [&](uint32_t lo, uint32_t hi, int t) -> uint64_t {
            uint64_t wv = 0;
            const int k0 = (64 * t) / kRunStep;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const int k = min(k0 + d, 63);
                const uint64_t m = ((uint64_t)(uint32_t)__shfl((int)hi, k, 64) << 32) |
                                   (uint32_t)__shfl((int)lo, k, 64);             // own bits 0 .. 53
                const int o = kRunStep * k - 64 * t;           // bit offset of the register in the word
                if (k0 + d < nreg && o < 64 && o > -kRunStep) wv |= o >= 0 ? (m << o) : (m >> -o);
            }
            return wv;
        };
        const int t = lane & 31;
        // (every lane shuffles the same plane's VGPRs: a shuffle reads the SOURCE lane's value)
        const uint64_t a0 = word(vPl, vPh, t), a1 = word(vUl, vUh, t);
        if (64 * t < len) wpos[w][lane < 32 ? t : kFeatWords + t] = lane < 32 ? a0 : a1;
        if (kEdge) {
            const uint64_t e2 = word(vEl, vEh, t);
            if (lane < 32 && 64 * t < len) wpos[w][2 * kFeatWords + t] = e2;
        }
    }
    bool fail = nrun > kRunMax;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");    // the loop's LDS writes before the reads
    __builtin_amdgcn_wave_barrier();
    int2 rj = make_int2(-1, len);
    int nj = 0;
    if (!fail && lane < nrun) {
        rj = wrun[w][lane];
        nj = (lane + 1 < nrun ? wrun[w][lane + 1].y : len) - rj.y;
        if (rj.x >= 0) {
            atomicAdd(&wnum[w][rj.x], 1);
            atomicAdd(&wlen[w][rj.x], nj);
            wst[w][rj.x] = rj.y;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const int cr = wlen[w][lane];                             // lane r: row r's own points
    fail = fail || __any(wnum[w][lane] > 1);
    if (fail) {                                               // uniform: a row in two runs, or too many runs
        if (lane == 0) irregular[lb] = kIrrGeneral;
        return;
    }
    int incl = cr;                                            // own-tile slot base of every row
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    const int base = incl - cr;
    const int bj = __shfl(base, rj.x & 63, 64);               // run lane j: its slot start
    const bool ident = __all(lane >= nrun || rj.x < 0 || bj == rj.y);   // slots = positions
    if (!ident) {                                             // uniform: move the runs' bits
        for (int j = 0; j < nrun; ++j) {
            const int r = __shfl(rj.x, j, 64), a = __shfl(rj.y, j, 64), n = __shfl(nj, j, 64);
            const int b = __shfl(bj, j, 64);
            if (r < 0 || n <= 0) continue;
            const int d0 = b >> 6, nd = ((b + n - 1) >> 6) - d0 + 1;
            for (int t = lane; t < kPl * nd; t += 64) {
                const int pl = t / nd, d = d0 + (t - pl * nd);
                const int lo = max(b, 64 * d), hi = min(b + n, 64 * d + 64);
                const uint64_t bits = bits_at(&wpos[w][pl * kFeatWords], lo - b + a, hi - lo, kFeatWords);
                if (bits)
                    __hip_atomic_fetch_or(&wslt[w][pl * kFeatWords + d], bits << (lo - 64 * d), __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    const unsigned long long* PL = ident ? &wpos[w][0] : &wslt[w][0];
    uint64_t* gb = gbits + ((int64_t)f * n_chunks + c) * kPW;
    for (int t = lane; t < kPl * kFeatWords; t += 64) gb[t] = PL[t];
    cnt[((int64_t)f * (n_chunks + 1) + c) * kMaxRows + lane] = cr;
    uint16_t* gi = gidx + idx_base(frame_off, f) + (int64_t)c * kBinChunk;
    if (!kDebug) {
        gi[lane] = (uint16_t)(cr > 0 ? wst[w][lane] : 0);     // the row's run start
    } else {                                                  // every slot's position (kIrrRunIdx)
        for (int j = 0; j < nrun; ++j) {
            const int r = __shfl(rj.x, j, 64), a = __shfl(rj.y, j, 64), n = __shfl(nj, j, 64);
            const int b = __shfl(bj, j, 64);
            if (r < 0) continue;
            for (int o = lane; o < n; o += 64) {
                gi[b + o] = (uint16_t)(a + o);
                if (curv_cm) curv_cm[s + b + o] = wcv[kDebug ? w : 0][a + o];
            }
        }
    }
    if (lane == 0) irregular[lb] = kDebug ? kIrrRunIdx : kIrrRun;
}

// Both kernels: kCurvNW chunks per work-group, the work-groups dealt over the 8 XCDs.
static dim3 wave_grid(const FeatLaunch& a) {
    const int64_t nblk = (int64_t)a.n_chunks * a.n_frames;
    const int64_t nwg = (nblk + kCurvNW - 1) / kCurvNW;
    return dim3((unsigned)((nwg + 7) / 8 * 8));
}

void launch_feat_wave_reg(const FeatLaunch& a, const FeatScratch& fs) {
    const FeatFrames& in = a.in;
    const ssf_config& cfg = a.cfg;
    kmark(a.s, "k_feat_wave_reg");
    dispatch_de(a.dbg, a.edge, [&](auto D, auto E) {
        hipLaunchKernelGGL((k_feat_wave_reg<decltype(D)::value, decltype(E)::value>), wave_grid(a), dim3(kCurvNT),
                           0, a.s, in.pts, in.stride, in.frame_off, a.n_frames, cfg.n_rows, a.n_chunks,
                           cfg.row_start, cfg.row_end, cfg.plane_min, a.es.min_curv,
                           reinterpret_cast<const RingTable*>(fs.rtab), fs.cnt, fs.gidx, fs.gbits, fs.curv_cm,
                           fs.irr, fs.lmap);
    });
}

void launch_feat_wave_run(const FeatLaunch& a, const FeatScratch& fs, bool all) {
    const FeatFrames& in = a.in;
    const ssf_config& cfg = a.cfg;
    kmark(a.s, "k_feat_wave_run");
    dispatch_de(a.dbg, a.edge, [&](auto D, auto E) {
        hipLaunchKernelGGL((k_feat_wave_run<decltype(D)::value, decltype(E)::value>), wave_grid(a), dim3(kCurvNT),
                           0, a.s, in.pts, in.stride, in.frame_off, a.n_frames, cfg.n_rows, a.n_chunks,
                           cfg.row_start, cfg.row_end, cfg.plane_min, a.es.min_curv, in.keep,
                           reinterpret_cast<const RingTable*>(fs.rtab), fs.cnt, fs.gidx, fs.gbits, fs.curv_cm,
                           fs.irr, all ? 1 : 0);
    });
}

}  // namespace ssf
