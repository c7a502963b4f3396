// feat_common.hpp -- what the feature-stage sources share (ring_table.hip, feat_bin.hip,
// feat_chunk.hip, feat_wave.hip, feat_select.hip, features.hip): the ring-id table and its device
// lookups, the window / tile constants and every tuning macro with its default (one value for
// all of them: build_variant passes its -D to every source), the chunk-major layout of the
// single-read stage, the 11-tap stencil and candidate flags, and the host dispatch that picks a
// kernel's <kDebug, kEdge> instantiation.
#pragma once
#include "ssf_device.hpp"
#include "ssf_internal.hpp"

#include <type_traits>

namespace ssf {

// ---- the ring id by table ---------------------------------------------------------------------
// frameFeature.cpp:57-73: `float angle = atan(point.z / sqrt(x*x + y*y)) * 180 / M_PI`, then the
// bin arithmetic of :60 / :63-71 and int() truncation.  C++ overload resolution allows two
// evaluations (oracle/ssf_oracle.c orc_ring_angle), selected by ssf_config.ring_chain:
//   SSF_RING_CHAIN_FLOAT (default): the float overloads libstdc++'s <math.h> puts at global scope
//     -- ratio = z / sqrtf(r2) (float), atanf, `* 180` in float, `/ M_PI` in double, to float;
//   SSF_RING_CHAIN_DOUBLE: only ::sqrt / ::atan(double) -- ratio = (double)z / sqrt((double)r2).
// Either way the row id is a monotone step function of ONE ratio (float or double).  The host
// evaluates the exact chain with the host libm (glibc atanf / atan, as oracle/ssf_oracle.c) once per
// context and cuts the ratio axis into kRingCells uniform cells (cell = clamp((ratio - r0) * inv),
// float ops, the same on both sides; a double ratio takes the cell of its float rounding); a cell
// holds at most two ids (cells are narrower than the narrowest bin), so per cell {the threshold
// where the second id starts (float; and as the exact double for the double chain), id below,
// id from there}.  The device computes the ratio exactly as the reference and does ONE table
// lookup and one compare: no atan on the device at all.
constexpr int kRingCells = 256;
constexpr int kRingChainFloat = SSF_RING_CHAIN_FLOAT, kRingChainDouble = SSF_RING_CHAIN_DOUBLE;
struct RingCell {
    float thr;          // ratios >= thr (float order) take id_b (double chain: thr rounded to float)
    int32_t ids;        // id_a (bits 0..7, signed), id_b (bits 8..15, signed)
};
struct RingTable {
    float r0, inv;
    RingCell cell[kRingCells];
    // per row, the float ratios of its interval [lo, hi) (the id is a monotone step function of
    // the ratio); an empty interval (lo >= hi) for a row that never occurs or is split.  Double
    // chain: the interval's ends rounded to float (the regular kernels' 1e-6 margins cover that)
    float rlo[kMaxRows], rhi[kMaxRows];
    int32_t chain, pad_;
    double dthr[kRingCells];   // per cell, the exact threshold of the double chain (float chain: thr)
};

SSF_DEV int ring_id_lookup(float ratio, float r0, float inv, const RingCell* T) {
    int ci = (int)((ratio - r0) * inv);          // v_cvt_i32_f32 saturates; NaN handled below
    ci = min(max(ci, 0), kRingCells - 1);
    const RingCell rc = T[ci];
    const int a = (int)(int8_t)(rc.ids & 0xff), b = (int)(int8_t)((rc.ids >> 8) & 0xff);
    const int id = ratio < rc.thr ? a : b;
    return ratio == ratio ? id : -1;             // 0 / 0 (a point at the origin): no row
}

// The reference's id from its exact ratio: the correctly rounded float z / sqrtf(r2) (float
// chain) or the correctly rounded double (double)z / sqrt((double)r2) against the cell's double
// threshold (double chain).  T: the cells (LDS or global), rt: the table (chain, dthr).
SSF_DEV int ring_id_exact(float x, float y, float z, float r0, float inv, const RingCell* T,
                          const RingTable* __restrict__ rt) {
    const float r2 = x * x + y * y;
    if (rt->chain != kRingChainDouble) return ring_id_lookup(z / sqrtf(r2), r0, inv, T);
    const double dr = (double)z / sqrt((double)r2);
    const float fr = (float)dr;
    int ci = (int)((fr - r0) * inv);
    ci = min(max(ci, 0), kRingCells - 1);
    const RingCell rc = T[ci];
    const int a = (int)(int8_t)(rc.ids & 0xff), b = (int)(int8_t)((rc.ids >> 8) & 0xff);
    const int id = dr < rt->dthr[ci] ? a : b;
    return dr == dr ? id : -1;
}

// The exact ratio needs a correctly rounded sqrt and divide (~30 instructions; f64 for the double
// chain).  The hardware reciprocal square root gives it to ~3e-7 relative (v_rsq_f32 1 ulp, one
// multiply, and the roundings of the exact form): that ratio takes the exact form's id unless a
// table threshold or a cell edge lies within 1e-6 of it (relative; a few in a million points), or
// r2 is tiny or not finite -- then the exact form decides (a rare, divergent branch).
SSF_DEV int ring_id_table(float x, float y, float z, float r0, float inv, const RingCell* T,
                          const RingTable* __restrict__ rt) {
    const float r2 = x * x + y * y;
    const float ra = z * __builtin_amdgcn_rsqf(r2);
    int ci = (int)((ra - r0) * inv);
    ci = min(max(ci, 0), kRingCells - 1);
    const RingCell rc = T[ci];
    const float m = 1e-6f * fmaxf(1.0f, fabsf(ra));
    const float tc = (ra - r0) * inv, fr = tc - floorf(tc);
    // every test evaluated (no short-circuit: one exec mask, one branch)
    const int near = (int)!(fabsf(ra - rc.thr) > m) | (int)!(fr > m * inv) | (int)!(fr < 1.0f - m * inv) |
                     (int)!(r2 > 1e-30f) | (int)!(r2 < 1e30f);
    const int a = (int)(int8_t)(rc.ids & 0xff), b = (int)(int8_t)((rc.ids >> 8) & 0xff);
    int id = ra < rc.thr ? a : b;
    if (near) id = ring_id_exact(x, y, z, r0, inv, T, rt);
    return id;
}

// ---- windows and tiles (k_bin_curv, k_feat_chunk; the wave kernels use the same halo) ---------
#ifndef SSF_CURV_HALO
#define SSF_CURV_HALO 384
#endif
#ifndef SSF_CURV_SUB
#define SSF_CURV_SUB 1
#endif
constexpr int kCurvHalo = SSF_CURV_HALO;                 // multiple of 64, <= kBinChunk
constexpr int kCurvSub = SSF_CURV_SUB;                   // binning chunks per work-group
constexpr int kCurvNT = 256 * kCurvSub;                  // threads per work-group
constexpr int kCurvNW = kCurvNT / 64;
constexpr int kCurvOwn = kBinChunk * kCurvSub;           // chunk points per work-group
constexpr int kWin = kCurvOwn + 2 * kCurvHalo;           // window points at most
constexpr int kWinQ = ((kWin + kCurvNW - 1) / kCurvNW + 63) / 64;   // 64-point steps per wave part
constexpr int kCE = ((kWin + kCurvNT - 1) / kCurvNT + 3) & ~3;      // tile entries per thread (12)
constexpr int kTileE = kCE * kCurvNT;                    // tile entries (>= kWin)
constexpr int kTilePad = 8;
static_assert(kCurvHalo % 64 == 0 && kCurvHalo <= kBinChunk, "halo");
static_assert(kWin < 4096 || kCurvSub > 1, "");
static_assert(kWin < 8192, "window positions and run lengths use 13 bits");
// tile entry classes (meta bits 24..25)
constexpr uint32_t kClsHalo = 0, kClsStencil = 1, kClsZero = 2, kClsOpen = 3;

// byte where frame f's flag bytes start: 64-byte aligned per frame, frames disjoint
// (buffer: total + 64 F + 64 bytes)
SSF_DEV int64_t flag_base(const int64_t* frame_off, int f) { return (frame_off[f] & ~(int64_t)63) + 64 * (int64_t)f; }

// the 11-tap sum of one coordinate, left to right (u[5] is the centre): frameFeature.cpp:88-97
SSF_DEV float tap11(const float* u) {
    float acc = u[0] + u[1];
#pragma unroll
    for (int k = 2; k < 11; ++k) acc = (k == 5) ? acc - 10.0f * u[5] : acc + u[k];
    return acc;
}

SSF_DEV uint8_t cand_flags(bool row_in, bool inner, float v, float plane_min, bool edge, float edge_min) {
    const float val = inner ? v : 0.0f;
    return (uint8_t)((row_in && val < plane_min) ? 1 : 0) |
           (uint8_t)((edge && row_in && inner && v > edge_min) ? 2 : 0);
}

// ---- the selection kernels (k_select, k_feat_select) -------------------------------------------
#ifndef SSF_SEL_THREADS
#define SSF_SEL_THREADS 1024
#endif
constexpr int kSelThreads = SSF_SEL_THREADS;
constexpr int kSelWordsLds = 6144;              // candidate words staged per array (48 KiB: 393k points)

// bit b of the result = bit `bit` of byte b of x (bytes' bits gathered by one multiply: the
// products 2^(8k + 7m + 7) never collide, so no carries)
SSF_DEV uint32_t pack8(uint64_t x, int bit) {
    return (uint32_t)((((x >> bit) & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56);
}

SSF_DEV uint64_t pack64(const uint64_t* b8, int bit) {
    uint64_t wv = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) wv |= (uint64_t)pack8(b8[k], bit) << (8 * k);
    return wv;
}

// ---- the single-read stage's chunk-major layout (feat_chunk.hip, feat_wave.hip, feat_select.hip)
#ifndef SSF_FEAT_WAVES
#define SSF_FEAT_WAVES 5                        // k_feat_chunk waves per SIMD (launch bound)
#endif
constexpr int kFeatMaxChunks = 128;              // 262144 points per frame (k_feat_select's LDS)
constexpr int kFeatPlanes = 3;                   // planar candidate, unresolved, edge candidate
constexpr int kFeatWords = kBinChunk / 64;       // 64-bit words per plane and chunk
constexpr uint8_t kFlP = 1, kFlU = 2, kFlE = 4;
// per (frame, chunk) block flag of the single-read stage: which kernel did the chunk and where
// k_feat_select finds a selected point's chunk position
//   kIrrRegular  k_feat_wave_reg: 64 x own column + the row's lane (lane map)
//   kIrrGeneral  not done yet -> k_feat_chunk_flagged, which writes the u16 position of every slot
//   kIrrRun      k_feat_wave_run: the row's run start (u16 at the chunk's first 64 index entries) + o
//   kIrrRunIdx   k_feat_wave_run with the debug outputs: the u16 position of every slot
constexpr uint8_t kIrrRegular = 0, kIrrGeneral = 1, kIrrRun = 2, kIrrRunIdx = 3;
static_assert(kCurvSub == 1 && kBinChunk == 2048, "own-tile slots and chunk positions use 11 bits");

// u16 index base of frame f: 64-entry aligned, frames disjoint with a gap of >= 33 entries (the
// chunk writes run up to 3 entries past the chunk's own points)
SSF_DEV int64_t idx_base(const int64_t* frame_off, int f) { return (frame_off[f] & ~(int64_t)31) + 64 * (int64_t)f; }

// ---- tuning macros of one kernel each ----------------------------------------------------------
#ifndef SSF_FEAT_WAVE_WAVES
#define SSF_FEAT_WAVE_WAVES 4                    // k_feat_wave_reg waves per SIMD (launch bound; 126 VGPRs)
#endif
#ifndef SSF_FEAT_WAVE_BLOCK
#define SSF_FEAT_WAVE_BLOCK 8                    // own columns per streamed block
#endif
#ifndef SSF_FEAT_RUN_WAVES
#define SSF_FEAT_RUN_WAVES 8                     // k_feat_wave_run waves per SIMD (launch bound)
#endif
#ifndef SSF_FEAT_RUN_PF
#define SSF_FEAT_RUN_PF 3                        // registers in flight per wave (r5ao: 3 0.0955 vs 4 0.0966 ms)
#endif
#ifndef SSF_SEL_OUT_U
#define SSF_SEL_OUT_U 1                          // r5az: 1 0.0477, 2 0.0495, 4 0.0515, 8 0.0556 ms
#endif

// ---- host: one kernel template, four instantiations --------------------------------------------
// f(std::bool_constant<kDebug>{}, std::bool_constant<kEdge>{}) for the launch's (dbg, edge): the
// one place a launcher's run-time pair becomes template arguments (a kernel with <kEdge> alone
// passes dbg = false and ignores the first).
template <class F>
inline void dispatch_de(bool dbg, bool edge, F&& f) {
    if (edge) { if (dbg) f(std::true_type{}, std::true_type{}); else f(std::false_type{}, std::true_type{}); }
    else { if (dbg) f(std::true_type{}, std::false_type{}); else f(std::false_type{}, std::false_type{}); }
}

}  // namespace ssf
