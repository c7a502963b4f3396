// abi_register.hip -- the registration entry points: batches of pairs (planes, or planes and
// edges), a chain of consecutive frames, one pair from host poses, the launch plan and the pose
// accumulation.
#include "abi_ctx.hpp"

static ssf::RegFrames frames(const float* xyzi, const int64_t* off, const int32_t* count) {
    return {reinterpret_cast<const float4*>(xyzi), off, count};
}

// What every registration entry fills alike: the pairs' clouds, the last frames' plane table and
// the record scratch (c->corr, sized by the caller).  The rest stays "not given".
static ssf::RegisterArgs register_args(ssf_ctx* c, ssf::RegFrames last, ssf::RegFrames curr, const float* normal,
                                       const uint8_t* valid, const float* sorted_xyzi, const int32_t* sorted_idx,
                                       const float* strip_xyzi, const int32_t* strip_head, int64_t max_m) {
    ssf::RegisterArgs a{};
    a.last = last; a.curr = curr;
    a.table.normal = normal; a.table.valid = valid;
    a.table.sorted = reinterpret_cast<const float4*>(sorted_xyzi); a.table.sidx = sorted_idx;
    a.table.strip_xyzi = reinterpret_cast<const float4*>(strip_xyzi); a.table.strip_head = strip_head;
    a.scratch.corr = c->corr.as<ssf::CorrRec>();
    a.max_m = max_m;
    return a;
}

extern "C" {

int32_t ssf_register_batch(ssf_ctx* c, void* stream, int32_t n_pairs, const float* d_last_xyzi,
                           const int64_t* d_last_off, const int32_t* d_last_count,
                           const float* d_last_normal, const uint8_t* d_last_valid,
                           const float* d_last_sorted_xyzi, const int32_t* d_last_sorted_idx,
                           const float* d_curr_xyzi, const int64_t* d_curr_off,
                           const int32_t* d_curr_count, int64_t curr_total_points,
                           int64_t max_plane_points, double* d_pose_rel, double* d_pose_abs,
                           double* d_log, int32_t* d_nlog, int32_t* d_ncorr, int32_t* d_nn,
                           const float* d_last_strip_xyzi, const int32_t* d_last_strip_head) {
    if (!c) return SSF_E_ARG;
    if (n_pairs < 0 || curr_total_points < 0 || max_plane_points < 0 ||
        (n_pairs > 0 && (!d_last_xyzi || !d_last_off || !d_last_count || !d_last_normal ||
                         !d_last_valid || !d_curr_xyzi || !d_curr_off || !d_curr_count || !d_pose_rel)))
        return fail(c, SSF_E_ARG, "register_batch: bad arguments");
    if (!strip_args_ok(d_last_strip_xyzi, d_last_strip_head, d_last_sorted_xyzi, d_last_sorted_idx))
        return fail(c, SSF_E_ARG, std::string("register_batch") + kStripArgsMsg);
    if (n_pairs == 0) return SSF_OK;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    SSF_TRY_HIP(c, c->corr.ensure(ssf::reg_corr_bytes(curr_total_points)), "alloc corr");
    SSF_TRY_HIP(c, c->cidx.ensure(ssf::reg_cidx_bytes(curr_total_points, n_pairs)), "alloc corr index");
    ProfScope prof(c, stream);
    ssf::RegisterArgs a = register_args(c, frames(d_last_xyzi, d_last_off, d_last_count),
                                        frames(d_curr_xyzi, d_curr_off, d_curr_count), d_last_normal,
                                        d_last_valid, d_last_sorted_xyzi, d_last_sorted_idx,
                                        d_last_strip_xyzi, d_last_strip_head, max_plane_points);
    a.pose.rel = d_pose_rel; a.pose.abs = d_pose_abs;
    a.out.log = d_log; a.out.nlog = d_nlog; a.out.ncorr = d_ncorr; a.out.nn = d_nn;
    a.scratch.nnv = c->cidx.as<int32_t>();
    a.scratch.ncompact = a.scratch.nnv + ssf::reg_queries(curr_total_points);
    return hip_rc(c, ssf::launch_register((hipStream_t)stream, c->cfg, n_pairs, a), "register launch");
}

int32_t ssf_register_plan(int32_t n_pairs, int64_t max_plane_points, int32_t with_edges,
                          ssf_launch_plan* out) {
    if (!out || n_pairs < 1 || max_plane_points < 0) return SSF_E_ARG;
    const ssf::RegisterPlan r = ssf::register_plan(n_pairs, max_plane_points, with_edges != 0);
    out->strip_path = r.strips;
    out->group_mode = r.coop;
    out->soa = r.soa;
    out->qsplit = r.qsplit;
    out->lds_cap = r.lds_cap;
    out->compacted = r.compacted;
    return SSF_OK;
}

int32_t ssf_register_chain(ssf_ctx* c, void* stream, int32_t n_pairs, const float* d_xyzi,
                           const int64_t* d_off, const int32_t* d_count, const float* d_normal,
                           const uint8_t* d_valid, const float* d_sorted_xyzi,
                           const int32_t* d_sorted_idx, int64_t total_points,
                           int64_t max_plane_points, const double* d_pose_init,
                           double* d_pose_seq, const double* d_pose_abs_init,
                           double* d_pose_abs_seq, int32_t* d_ncorr,
                           const float* d_strip_xyzi, const int32_t* d_strip_head) {
    if (!c) return SSF_E_ARG;
    if (n_pairs < 0 || total_points < 0 || max_plane_points < 0 ||
        (n_pairs > 0 && (!d_xyzi || !d_off || !d_count || !d_normal || !d_valid || !d_pose_init ||
                         !d_pose_seq)) ||
        (!d_pose_abs_init != !d_pose_abs_seq))
        return fail(c, SSF_E_ARG, "register_chain: bad arguments");
    if (!strip_args_ok(d_strip_xyzi, d_strip_head, d_sorted_xyzi, d_sorted_idx))
        return fail(c, SSF_E_ARG, std::string("register_chain") + kStripArgsMsg);
    if (n_pairs == 0) return SSF_OK;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    SSF_TRY_HIP(c, c->corr.ensure(ssf::reg_corr_bytes(total_points)), "alloc corr");
    ProfScope prof(c, stream);
    // pair k = (frame k, frame k + 1) of the same arrays: its warm start is pair k - 1's output
    // slot (lidarOdometry_onlyPC.cpp:164,251-252), read in place by the association and the
    // solve -- no copy between the links, two launches per pair, all enqueued here
    for (int k = 0; k < n_pairs; ++k) {            // no log, no 1-NN output, no compaction scratch
        ssf::RegisterArgs a = register_args(c, frames(d_xyzi, d_off + k, d_count + k),
                                            frames(d_xyzi, d_off + k + 1, d_count + k + 1), d_normal, d_valid,
                                            d_sorted_xyzi, d_sorted_idx, d_strip_xyzi, d_strip_head,
                                            max_plane_points);
        a.pose.in = k == 0 ? d_pose_init : d_pose_seq + 7 * (k - 1);
        a.pose.rel = d_pose_seq + 7 * k;
        if (d_pose_abs_seq) {
            a.pose.abs_in = k == 0 ? d_pose_abs_init : d_pose_abs_seq + 7 * (k - 1);
            a.pose.abs = d_pose_abs_seq + 7 * k;
        }
        if (d_ncorr) a.out.ncorr = d_ncorr + k;
        SSF_TRY_HIP(c, ssf::launch_register((hipStream_t)stream, c->cfg, 1, a), "register_chain launch");
    }
    return SSF_OK;
}

int32_t ssf_register_batch_edges(ssf_ctx* c, void* stream, int32_t n_pairs,
                                 const float* d_last_xyzi, const int64_t* d_last_off,
                                 const int32_t* d_last_count, const float* d_last_normal,
                                 const uint8_t* d_last_valid, const float* d_last_sorted_xyzi,
                                 const int32_t* d_last_sorted_idx, const float* d_curr_xyzi,
                                 const int64_t* d_curr_off, const int32_t* d_curr_count,
                                 int64_t curr_total_points, int64_t max_plane_points,
                                 const float* d_last_edge_xyzi, const int64_t* d_last_edge_off,
                                 const int32_t* d_last_edge_count, const float* d_last_line,
                                 const uint8_t* d_last_line_valid, const float* d_curr_edge_xyzi,
                                 const int64_t* d_curr_edge_off, const int32_t* d_curr_edge_count,
                                 int64_t curr_edge_total, int64_t max_edge_points,
                                 double* d_pose_rel, double* d_pose_abs, double* d_log,
                                 int32_t* d_nlog, int32_t* d_ncorr, int32_t* d_ncorr_edge,
                                 const float* d_last_strip_xyzi, const int32_t* d_last_strip_head) {
    if (!c) return SSF_E_ARG;
    if (!strip_args_ok(d_last_strip_xyzi, d_last_strip_head, d_last_sorted_xyzi, d_last_sorted_idx))
        return fail(c, SSF_E_ARG, std::string("register_batch_edges") + kStripArgsMsg);
    if (n_pairs < 0 || curr_total_points < 0 || max_plane_points < 0 || curr_edge_total < 0 ||
        max_edge_points < 0 ||
        (n_pairs > 0 && (!d_last_xyzi || !d_last_off || !d_last_count || !d_last_normal ||
                         !d_last_valid || !d_curr_xyzi || !d_curr_off || !d_curr_count || !d_pose_rel ||
                         !d_last_edge_xyzi || !d_last_edge_off || !d_last_edge_count || !d_last_line ||
                         !d_last_line_valid || !d_curr_edge_xyzi || !d_curr_edge_off || !d_curr_edge_count)))
        return fail(c, SSF_E_ARG, "register_batch_edges: bad arguments");
    if (n_pairs == 0) return SSF_OK;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    SSF_TRY_HIP(c, c->corr.ensure(ssf::reg_corr_bytes(curr_total_points)), "alloc corr");
    SSF_TRY_HIP(c, c->ecorr.ensure(ssf::reg_corr_bytes(curr_edge_total)), "alloc edge corr");
    if (max_edge_points == 0) {
        // no edge point anywhere: the edge records are never read, but their counts are
        SSF_TRY_HIP(c, hipMemsetAsync(c->ecorr.p, 0, sizeof(ssf::CorrRec), (hipStream_t)stream), "zero ecorr");
    }
    ProfScope prof(c, stream);
    const ssf::EdgeReg er{reinterpret_cast<const float4*>(d_last_edge_xyzi), d_last_edge_off,
                          d_last_edge_count, d_last_line, d_last_line_valid,
                          reinterpret_cast<const float4*>(d_curr_edge_xyzi), d_curr_edge_off,
                          d_curr_edge_count, max_edge_points, c->ecorr.as<ssf::CorrRec>(), d_ncorr_edge};
    // no 1-NN output, no compaction scratch
    ssf::RegisterArgs a = register_args(c, frames(d_last_xyzi, d_last_off, d_last_count),
                                        frames(d_curr_xyzi, d_curr_off, d_curr_count), d_last_normal,
                                        d_last_valid, d_last_sorted_xyzi, d_last_sorted_idx,
                                        d_last_strip_xyzi, d_last_strip_head, max_plane_points);
    a.pose.rel = d_pose_rel; a.pose.abs = d_pose_abs;
    a.out.log = d_log; a.out.nlog = d_nlog; a.out.ncorr = d_ncorr;
    a.edge = &er;
    return hip_rc(c, ssf::launch_register((hipStream_t)stream, c->cfg, n_pairs, a), "register_edges launch");
}

int32_t ssf_register_pair(ssf_ctx* c, void* stream, const float* d_last_xyzi, int64_t m_last,
                          const float* d_curr_xyzi, int64_t m_curr, const double* h_q_init,
                          const double* h_t_init, double* h_q_out, double* h_t_out,
                          ssf_step_log* log) {
    if (!c) return SSF_E_ARG;
    if (m_last < 0 || m_curr < 0 || m_last > INT32_MAX || m_curr > INT32_MAX || !h_q_init ||
        !h_t_init || !h_q_out || !h_t_out || (m_last > 0 && !d_last_xyzi) ||
        (m_curr > 0 && !d_curr_xyzi) || (log && log->cap > 0 && !log->steps))
        return fail(c, SSF_E_ARG, "register_pair: bad arguments");
    double pose[7] = {h_q_init[0], h_q_init[1], h_q_init[2], h_q_init[3], h_t_init[0], h_t_init[1], h_t_init[2]};
    if (log) { log->n_steps = 0; log->n_corr = -1; }
    if (m_last <= 10 || m_curr == 0) {             // :158 -- no residuals, the warm start stands
        for (int k = 0; k < 4; ++k) h_q_out[k] = pose[k];
        for (int k = 0; k < 3; ++k) h_t_out[k] = pose[4 + k];
        if (log && m_last > 10) log->n_corr = 0;
        return SSF_OK;
    }
    hipStream_t s = (hipStream_t)stream;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    const int max_iter = c->cfg.max_iter;
    const int64_t mx = std::max(m_last, m_curr);
    // scratch layout (8-byte aligned pieces): offsets, counts, pose, log doubles, nlog/ncorr,
    // normals, valid, sorted cloud (16 B aligned), sorted index
    auto al = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t o_off = 0, o_cnt = al(o_off + 4 * sizeof(int64_t)), o_pose = al(o_cnt + 4 * sizeof(int32_t));
    const size_t o_log = al(o_pose + 7 * sizeof(double));
    const size_t o_nl = al(o_log + (size_t)std::max(max_iter, 1) * 10 * sizeof(double));
    const size_t o_nrm = al(o_nl + 2 * sizeof(int32_t));
    const size_t o_val = al(o_nrm + 3 * sizeof(float) * (size_t)m_last);
    const size_t o_srt = al(o_val + (size_t)m_last);
    const size_t o_sid = al(o_srt + sizeof(float4) * (size_t)m_last);
    const size_t o_sim = al(o_sid + sizeof(int32_t) * (size_t)m_last);
    const size_t o_shd = al(o_sim + sizeof(float4) * (size_t)m_last);
    const size_t bytes = al(o_shd + sizeof(int32_t) * (size_t)m_last);
    SSF_TRY_HIP(c, c->pair.ensure(bytes), "alloc pair scratch");
    char* P = c->pair.as<char>();
    int64_t* d_off = reinterpret_cast<int64_t*>(P + o_off);     // [0, m_last] and [0, m_curr]
    int32_t* d_cnt = reinterpret_cast<int32_t*>(P + o_cnt);
    double* d_pose = reinterpret_cast<double*>(P + o_pose);
    double* d_log = reinterpret_cast<double*>(P + o_log);
    int32_t* d_nl = reinterpret_cast<int32_t*>(P + o_nl);
    float* d_nrm = reinterpret_cast<float*>(P + o_nrm);
    uint8_t* d_val = reinterpret_cast<uint8_t*>(P + o_val);
    float* d_srt = reinterpret_cast<float*>(P + o_srt);
    int32_t* d_sid = reinterpret_cast<int32_t*>(P + o_sid);
    float* d_sim = reinterpret_cast<float*>(P + o_sim);        // the table's strip image
    int32_t* d_shd = reinterpret_cast<int32_t*>(P + o_shd);
    struct { int64_t off[4]; int32_t cnt[4]; double pose[7]; } h;
    h.off[0] = 0; h.off[1] = m_last; h.off[2] = 0; h.off[3] = m_curr;
    h.cnt[0] = (int32_t)m_last; h.cnt[1] = (int32_t)m_curr; h.cnt[2] = h.cnt[3] = 0;
    for (int k = 0; k < 7; ++k) h.pose[k] = pose[k];
    SSF_TRY_HIP(c, hipMemcpyAsync(d_off, h.off, sizeof(h.off), hipMemcpyHostToDevice, s), "H2D off");
    SSF_TRY_HIP(c, hipMemcpyAsync(d_cnt, h.cnt, sizeof(h.cnt), hipMemcpyHostToDevice, s), "H2D counts");
    SSF_TRY_HIP(c, hipMemcpyAsync(d_pose, h.pose, sizeof(h.pose), hipMemcpyHostToDevice, s), "H2D pose");
    int32_t rc = ssf_plane_table_batch(c, stream, 1, d_last_xyzi, d_off, d_cnt, mx, d_nrm, d_val, d_srt, d_sid,
                                       d_sim, d_shd);
    if (rc) return rc;
    rc = ssf_register_batch(c, stream, 1, d_last_xyzi, d_off, d_cnt, d_nrm, d_val, d_srt, d_sid,
                            d_curr_xyzi, d_off + 2, d_cnt + 1, m_curr, mx, d_pose, nullptr,
                            d_log, d_nl, d_nl + 1, nullptr, d_sim, d_shd);
    if (rc) return rc;
    std::vector<double> hl((size_t)std::max(max_iter, 1) * 10);
    int32_t hn[2] = {0, 0};
    SSF_TRY_HIP(c, hipMemcpyAsync(h.pose, d_pose, sizeof(h.pose), hipMemcpyDeviceToHost, s), "D2H pose");
    SSF_TRY_HIP(c, hipMemcpyAsync(hn, d_nl, sizeof(hn), hipMemcpyDeviceToHost, s), "D2H nlog");
    if (log && log->cap > 0)
        SSF_TRY_HIP(c, hipMemcpyAsync(hl.data(), d_log, sizeof(double) * hl.size(), hipMemcpyDeviceToHost, s), "D2H log");
    SSF_TRY_HIP(c, hipStreamSynchronize(s), "sync");
    for (int k = 0; k < 4; ++k) h_q_out[k] = h.pose[k];
    for (int k = 0; k < 3; ++k) h_t_out[k] = h.pose[4 + k];
    if (log) {
        log->n_corr = hn[1];
        const int n = std::min(std::min(hn[0], max_iter), std::max(log->cap, 0));
        for (int i = 0; i < n; ++i) {
            const double* r = &hl[(size_t)i * 10];
            ssf_step& st = log->steps[i];
            for (int k = 0; k < 4; ++k) st.q[k] = r[k];
            for (int k = 0; k < 3; ++k) st.t[k] = r[4 + k];
            st.cost = r[7];
            st.status = (int32_t)r[8];
            st.pad = 0;
            st.radius = r[9];
        }
        log->n_steps = n;
    }
    return SSF_OK;
}

int32_t ssf_accumulate_sequence(ssf_ctx* c, void* stream, int32_t n, const double* d_rel,
                                const double* h_start, double* d_abs) {
    if (!c) return SSF_E_ARG;
    if (n < 0 || (n > 0 && (!d_rel || !d_abs))) return fail(c, SSF_E_ARG, "accumulate: bad arguments");
    if (n == 0) return SSF_OK;
    hipStream_t s = (hipStream_t)stream;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    const double* d_start = nullptr;
    if (h_start) {
        SSF_TRY_HIP(c, c->start1.ensure(sizeof(double) * 8), "alloc start");
        SSF_TRY_HIP(c, hipMemcpyAsync(c->start1.p, h_start, sizeof(double) * 7, hipMemcpyHostToDevice, s), "H2D start");
        d_start = c->start1.as<double>();
    }
    ProfScope prof(c, stream);
    SSF_TRY_HIP(c, ssf::launch_accumulate(s, n, d_rel, d_start, d_abs), "accumulate launch");
    if (h_start) SSF_TRY_HIP(c, hipStreamSynchronize(s), "sync start");
    return SSF_OK;
}

}  // extern "C"
