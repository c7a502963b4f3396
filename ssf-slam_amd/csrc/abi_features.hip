// abi_features.hip -- the feature-stage entry points: plane / edge extraction and the plane and
// line tables the registration reads.
#include "abi_ctx.hpp"

int32_t ensure_features(ssf_ctx* c, int32_t n_frames, int64_t total, int64_t max_pts) {
    const int R = c->cfg.n_rows;
    const int64_t n_chunks = (max_pts + ssf::kBinChunk - 1) / ssf::kBinChunk;
    SSF_TRY_HIP(c, c->rid.ensure((size_t)std::max<int64_t>(total, 1)), "alloc rid");
    SSF_TRY_HIP(c, c->hist.ensure(sizeof(int32_t) * (size_t)std::max<int64_t>(n_frames * n_chunks * R, 1)), "alloc hist");
    SSF_TRY_HIP(c, c->ring_off.ensure(sizeof(int32_t) * (size_t)n_frames * (R + 1)), "alloc ring_off");
    // ring index (input index per ring position), per-row selection slots (indexInRow at ring
    // positions, k_select), candidate flag bytes, curvature fix-up list
    SSF_TRY_HIP(c, c->ring_xyzi.ensure(sizeof(int32_t) * (size_t)std::max<int64_t>(total, 1)), "alloc ring index");
    SSF_TRY_HIP(c, c->sel.ensure(sizeof(int32_t) * (size_t)std::max<int64_t>(total, 1)), "alloc sel");
    SSF_TRY_HIP(c, c->sel_cnt.ensure(ssf::flag_bytes(total, n_frames)), "alloc cand flags");
    SSF_TRY_HIP(c, c->fix.ensure(ssf::fix_bytes(total, n_frames)), "alloc curvature fix-up list");
    if (!c->rtab_ready) {                           // every feature path looks ring ids up in it
        std::vector<char> h(ssf::ring_table_bytes());
        const int rc = ssf::build_ring_table(R, c->cfg.ring_chain, h.data());
        if (rc) return fail(c, SSF_E_ARG, "ring-id table: build failed (" + std::to_string(rc) + ")");
        SSF_TRY_HIP(c, c->rtab.ensure(h.size()), "alloc ring table");
        SSF_TRY_HIP(c, hipMemcpy(c->rtab.p, h.data(), h.size(), hipMemcpyHostToDevice), "H2D ring table");
        c->rtab_ready = true;
    }
    if (ssf::feat_single_read(max_pts)) {
        SSF_TRY_HIP(c, c->fcnt.ensure(ssf::feat_cnt_bytes(n_frames, max_pts)), "alloc feature counts");
        SSF_TRY_HIP(c, c->fidx.ensure(ssf::feat_idx_bytes(total, n_frames)), "alloc feature index");
        SSF_TRY_HIP(c, c->fbits.ensure(ssf::feat_bits_bytes(n_frames, max_pts)), "alloc feature bits");
        SSF_TRY_HIP(c, c->firr.ensure(ssf::feat_irr_bytes(n_frames, max_pts)), "alloc feature block flags");
        SSF_TRY_HIP(c, c->flmap.ensure(ssf::feat_lmap_bytes(n_frames, max_pts)), "alloc feature lane maps");
    }
    return SSF_OK;
}

static int32_t extract_planes_impl(ssf_ctx* c, void* stream, int32_t n_frames, const float* d_pts,
                                   int32_t point_stride, const int64_t* d_frame_off,
                                   int64_t total_points, int64_t max_frame_points,
                                   const uint8_t* d_keep, float* d_plane_xyzi,
                                   int32_t* d_plane_count, float* d_ring_xyzi, int32_t* d_ring_off,
                                   float* d_curv, float* d_edge_xyzi = nullptr,
                                   int32_t* d_edge_count = nullptr) {
    if (!c) return SSF_E_ARG;
    if (n_frames < 0 || point_stride < 3 || total_points < 0 || max_frame_points < 0 ||
        (n_frames > 0 && (!d_pts || !d_frame_off || !d_plane_xyzi || !d_plane_count)))
        return fail(c, SSF_E_ARG, "extract_planes_batch: bad arguments");
    if (max_frame_points >= ((int64_t)1 << 24))
        return fail(c, SSF_E_ARG, "extract_planes_batch: frames of at most 16777215 points (24-bit ring positions)");
    if (n_frames == 0) return SSF_OK;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    int32_t rc = ensure_features(c, n_frames, total_points, max_frame_points);
    if (rc) return rc;
    ssf::EdgeSel es{};
    const bool edges = d_edge_xyzi != nullptr;
    if (edges) {
        SSF_TRY_HIP(c, c->esel.ensure(sizeof(int32_t) * (size_t)std::max<int64_t>(total_points, 1)), "alloc esel");
        es = ssf::EdgeSel{c->ecfg.edge_min, c->ecfg.edge_span,
                          c->esel.as<int32_t>(), reinterpret_cast<float4*>(d_edge_xyzi), d_edge_count};
    }
    float4* ring4 = reinterpret_cast<float4*>(d_ring_xyzi);   // debug output only (nullable)
    if ((ring4 || d_curv) && ssf::feat_single_read(max_frame_points))
        SSF_TRY_HIP(c, c->fcurv.ensure(sizeof(float) * (size_t)std::max<int64_t>(total_points, 1)), "alloc chunk curvature");
    ssf::FeatScratch fs{c->rtab.p, c->fcnt.as<int32_t>(), c->fidx.as<uint16_t>(), c->fbits.as<uint64_t>(),
                        c->fcurv.as<float>(), c->firr.as<uint8_t>(), c->flmap.as<uint8_t>()};
    ssf::BinScratch bin{};
    bin.rid = c->rid.as<int8_t>(); bin.hist = c->hist.as<int32_t>();
    bin.ring_idx = c->ring_xyzi.as<int32_t>(); bin.flags = c->sel_cnt.as<uint8_t>(); bin.fix = c->fix.p;
    ssf::FeatFrames in{};
    in.pts = d_pts; in.stride = point_stride; in.frame_off = d_frame_off;
    in.max_pts = max_frame_points; in.keep = d_keep;
    ssf::FeatOut out{};
    out.plane = reinterpret_cast<float4*>(d_plane_xyzi); out.plane_count = d_plane_count;
    out.ring_off = d_ring_off ? d_ring_off : c->ring_off.as<int32_t>();
    out.ring_xyzi = ring4; out.curv = d_curv;
    const ssf::EdgeSel* edge = edges ? &es : nullptr;
    ProfScope prof(c, stream);
    return hip_rc(c, ssf::launch_extract_planes((hipStream_t)stream, c->cfg, n_frames, in, out,
                                              c->sel.as<int32_t>(), bin, fs, edge), "extract_planes launch");
}

extern "C" {

int32_t ssf_extract_planes_batch(ssf_ctx* c, void* stream, int32_t n_frames, const float* d_pts,
                                 int32_t point_stride, const int64_t* d_frame_off,
                                 int64_t total_points, int64_t max_frame_points,
                                 float* d_plane_xyzi, int32_t* d_plane_count, float* d_ring_xyzi,
                                 int32_t* d_ring_off, float* d_curv) {
    return extract_planes_impl(c, stream, n_frames, d_pts, point_stride, d_frame_off, total_points,
                               max_frame_points, nullptr, d_plane_xyzi, d_plane_count, d_ring_xyzi,
                               d_ring_off, d_curv);
}

int32_t ssf_extract_planes_batch_masked(ssf_ctx* c, void* stream, int32_t n_frames,
                                        const float* d_pts, int32_t point_stride,
                                        const int64_t* d_frame_off, int64_t total_points,
                                        int64_t max_frame_points, const uint8_t* d_keep,
                                        float* d_plane_xyzi, int32_t* d_plane_count,
                                        float* d_ring_xyzi, int32_t* d_ring_off, float* d_curv) {
    if (c && n_frames > 0 && !d_keep) return fail(c, SSF_E_ARG, "extract_planes_batch_masked: null keep mask");
    return extract_planes_impl(c, stream, n_frames, d_pts, point_stride, d_frame_off, total_points,
                               max_frame_points, d_keep, d_plane_xyzi, d_plane_count, d_ring_xyzi,
                               d_ring_off, d_curv);
}

int32_t ssf_extract_features_batch(ssf_ctx* c, void* stream, int32_t n_frames, const float* d_pts,
                                   int32_t point_stride, const int64_t* d_frame_off,
                                   int64_t total_points, int64_t max_frame_points,
                                   const uint8_t* d_keep, float* d_plane_xyzi,
                                   int32_t* d_plane_count, float* d_edge_xyzi,
                                   int32_t* d_edge_count) {
    if (c && n_frames > 0 && (!d_edge_xyzi || !d_edge_count))
        return fail(c, SSF_E_ARG, "extract_features_batch: null edge outputs");
    return extract_planes_impl(c, stream, n_frames, d_pts, point_stride, d_frame_off, total_points,
                               max_frame_points, d_keep, d_plane_xyzi, d_plane_count, nullptr,
                               nullptr, nullptr, d_edge_xyzi, d_edge_count);
}

int32_t ssf_edge_table_batch(ssf_ctx* c, void* stream, int32_t n_frames, const float* d_edge_xyzi,
                             const int64_t* d_frame_off, const int32_t* d_edge_count,
                             int64_t max_edge_points, float* d_line, uint8_t* d_line_valid) {
    if (!c) return SSF_E_ARG;
    if (n_frames < 0 || max_edge_points < 0 ||
        (n_frames > 0 && (!d_edge_xyzi || !d_frame_off || !d_edge_count || !d_line || !d_line_valid)))
        return fail(c, SSF_E_ARG, "edge_table_batch: bad arguments");
    if (n_frames == 0) return SSF_OK;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    ProfScope prof(c, stream);
    return hip_rc(c, ssf::launch_edge_table((hipStream_t)stream, c->ecfg, n_frames,
                                         reinterpret_cast<const float4*>(d_edge_xyzi), d_frame_off,
                                         d_edge_count, max_edge_points, d_line, d_line_valid), "edge_table launch");
}

int32_t ssf_extract_planes(ssf_ctx* c, void* stream, const float* d_pts, int64_t n,
                           int32_t point_step_bytes, int32_t xyz_offset_bytes, float* d_out_xyzi,
                           int64_t* h_out_m, int64_t out_cap) {
    if (!c) return SSF_E_ARG;
    if (n < 0 || !h_out_m || point_step_bytes < 12 || point_step_bytes % 4 || xyz_offset_bytes < 0 ||
        xyz_offset_bytes % 4 || xyz_offset_bytes + 12 > point_step_bytes || (n > 0 && (!d_pts || !d_out_xyzi)))
        return fail(c, SSF_E_ARG, "extract_planes: bad arguments");
    *h_out_m = 0;
    if (n == 0) return SSF_OK;
    hipStream_t s = (hipStream_t)stream;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    SSF_TRY_HIP(c, c->off1.ensure(2 * sizeof(int64_t)), "alloc off1");
    SSF_TRY_HIP(c, c->cnt1.ensure(sizeof(int32_t)), "alloc cnt1");
    SSF_TRY_HIP(c, c->plane1.ensure(sizeof(float4) * (size_t)n), "alloc plane1");
    const int64_t off[2] = {0, n};
    SSF_TRY_HIP(c, hipMemcpyAsync(c->off1.p, off, sizeof(off), hipMemcpyHostToDevice, s), "H2D off");
    const float* base = reinterpret_cast<const float*>(reinterpret_cast<const char*>(d_pts) + xyz_offset_bytes);
    int32_t rc = ssf_extract_planes_batch(c, stream, 1, base, point_step_bytes / 4, c->off1.as<int64_t>(), n, n,
                                          c->plane1.as<float>(), c->cnt1.as<int32_t>(), nullptr, nullptr, nullptr);
    if (rc) return rc;
    int32_t m = 0;
    SSF_TRY_HIP(c, hipMemcpyAsync(&m, c->cnt1.p, sizeof(m), hipMemcpyDeviceToHost, s), "D2H count");
    SSF_TRY_HIP(c, hipStreamSynchronize(s), "sync");
    *h_out_m = m;
    if (m > out_cap) return fail(c, SSF_E_CAPACITY, "extract_planes: " + std::to_string(m) + " plane points exceed out_cap");
    if (m > 0)
        SSF_TRY_HIP(c, hipMemcpyAsync(d_out_xyzi, c->plane1.p, sizeof(float4) * (size_t)m, hipMemcpyDeviceToDevice, s), "D2D planes");
    return SSF_OK;
}

int32_t ssf_plane_table_batch(ssf_ctx* c, void* stream, int32_t n_frames, const float* d_plane_xyzi,
                              const int64_t* d_frame_off, const int32_t* d_plane_count,
                              int64_t max_plane_points, float* d_normal, uint8_t* d_valid,
                              float* d_sorted_xyzi, int32_t* d_sorted_idx, float* d_strip_xyzi,
                              int32_t* d_strip_head) {
    if (!c) return SSF_E_ARG;
    if (n_frames < 0 || max_plane_points < 0 ||
        (n_frames > 0 && (!d_plane_xyzi || !d_frame_off || !d_plane_count || !d_normal || !d_valid)))
        return fail(c, SSF_E_ARG, "plane_table_batch: bad arguments");
    if (!strip_args_ok(d_strip_xyzi, d_strip_head, d_sorted_xyzi, d_sorted_idx))
        return fail(c, SSF_E_ARG, std::string("plane_table_batch") + kStripArgsMsg);
    if (n_frames == 0) return SSF_OK;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    ProfScope prof(c, stream);
    return hip_rc(c, ssf::launch_plane_table((hipStream_t)stream, c->cfg, n_frames,
                                           reinterpret_cast<const float4*>(d_plane_xyzi), d_frame_off,
                                           d_plane_count, max_plane_points, d_normal, d_valid,
                                           reinterpret_cast<float4*>(d_sorted_xyzi), d_sorted_idx,
                                           reinterpret_cast<float4*>(d_strip_xyzi), d_strip_head), "plane_table launch");
}

}  // extern "C"
