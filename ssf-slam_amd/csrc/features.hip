// features.hip -- frameFeature::cloudHandler (src/frameFeature.cpp:35-139) on gfx950: the scratch
// sizes of the feature stage and launch_extract_planes, which picks the path of a batch of frames
// and calls the stages' launchers in order.
//   frames of at most kFeatMaxChunks chunks (262144 points) -- the single-read stage, the points
//   read once:
//     k_feat_wave_reg       unmasked 64-beam frames: the regular windows of an azimuth-ordered
//                           scan, one wave per chunk; flags the others        (feat_wave.hip)
//     k_feat_wave_run       the chunks left (all of them without the kernel above) whose rows
//                           come as runs of consecutive inputs                (feat_wave.hip)
//     k_feat_chunk_flagged  the chunks still flagged, any layout; k_feat_chunk does every chunk
//                           when neither wave kernel can run                  (feat_chunk.hip)
//     k_feat_select         one work-group per frame: the chunks' candidates to ring order, the
//                           greedy spacing rule, the plane (and edge) clouds  (feat_select.hip)
//     k_feat_debug          debug outputs only: ring-ordered cloud, curvature (feat_select.hip)
//   larger frames -- the binned stage: k_bin_count, k_bin_scan, k_bin_curv, k_select (feat_bin.hip)
// Every path needs the ring-id table (feat_common.hpp; built on the host by ring_table.hip).
#include "feat_common.hpp"

#include <algorithm>

namespace ssf {

size_t feat_idx_bytes(int64_t total, int n_frames) { return sizeof(uint16_t) * (size_t)(total + 64 * (int64_t)n_frames + 64); }
size_t feat_bits_bytes(int n_frames, int64_t max_pts) {
    const int64_t nc = (max_pts + kBinChunk - 1) / kBinChunk;
    return sizeof(uint64_t) * (size_t)std::max<int64_t>(1, (int64_t)n_frames * nc) * kFeatPlanes * kFeatWords;
}
size_t feat_cnt_bytes(int n_frames, int64_t max_pts) {
    const int64_t nc = (max_pts + kBinChunk - 1) / kBinChunk;
    return sizeof(int32_t) * (size_t)std::max(1, n_frames) * (nc + 1) * kMaxRows;
}
size_t feat_lmap_bytes(int n_frames, int64_t max_pts) {
    const int64_t nc = (max_pts + kBinChunk - 1) / kBinChunk;
    return (size_t)std::max<int64_t>(1, (int64_t)n_frames * nc) * kMaxRows;
}
size_t feat_irr_bytes(int n_frames, int64_t max_pts) {
    const int64_t nc = (max_pts + kBinChunk - 1) / kBinChunk;
    return (size_t)std::max<int64_t>(16, ((int64_t)n_frames * nc + 15) & ~(int64_t)15);
}
bool feat_single_read(int64_t max_pts) {
    return (max_pts + kBinChunk - 1) / kBinChunk <= kFeatMaxChunks;
}

size_t flag_bytes(int64_t total, int n_frames) { return (size_t)(total + 64 * (int64_t)n_frames + 64); }
// per-frame fix-up counts (64-byte aligned block), then the entries at the frame offsets
size_t fix_bytes(int64_t total, int n_frames) { return fix_head(n_frames) + sizeof(int32_t) * (size_t)(total + 1); }

hipError_t launch_extract_planes(hipStream_t s, const ssf_config& cfg, int n_frames,
                                 const FeatFrames& in, const FeatOut& out, int32_t* sel,
                                 const BinScratch& bin, const FeatScratch& fs, const EdgeSel* edge) {
    const int n_chunks = (int)((in.max_pts + kBinChunk - 1) / kBinChunk);
    if (n_frames <= 0) return hipSuccess;
    if (cfg.n_rows > kMaxRows) return hipErrorInvalidValue;
    if (in.max_pts >= (int64_t)1 << 24) return hipErrorInvalidValue;   // ring positions: 24 bits
    const bool dbg = out.curv != nullptr || out.ring_xyzi != nullptr;
    const FeatLaunch a{s, cfg, n_frames, n_chunks, in, out, sel, dbg, edge != nullptr,
                       edge ? *edge : EdgeSel{0.f, 1, nullptr, nullptr, nullptr}};
    if (!feat_single_read(in.max_pts) || n_chunks == 0) {
        const hipError_t e = launch_feat_bin(a, bin, fs.rtab);
        return e != hipSuccess ? e : hipGetLastError();
    }
    // unmasked 64-beam frames: the regular-window kernel first (it flags the blocks it leaves)
    const bool regular = !in.keep && cfg.n_rows == kMaxRows && fs.irr && fs.lmap &&
                         in.stride <= 4096;                  // k_feat_wave_reg: 32-bit window offsets
    // the run kernel next, for the chunks k_feat_wave_reg left (every chunk when it did not
    // run: masked frames, 16 beams); then k_feat_chunk for the rest
    const bool run = fs.irr && in.stride <= 4096;
    FeatScratch u = fs;                                       // what this launch uses of it
    u.curv_cm = dbg ? fs.curv_cm : nullptr;
    u.irr = (regular || run) ? fs.irr : nullptr;
    u.lmap = regular ? fs.lmap : nullptr;
    if (regular) launch_feat_wave_reg(a, u);
    if (run) launch_feat_wave_run(a, u, !regular);
    launch_feat_chunk(a, u);
    launch_feat_select(a, u);
    if (dbg) launch_feat_debug(a, u);
    return hipGetLastError();
}

}  // namespace ssf
