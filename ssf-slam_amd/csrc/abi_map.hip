// abi_map.hip -- the map back-end's entry points: voxel grid, cloud transform, ICP, Scan Context
// (describe, match, top-k match) and the pose-graph solver with its defaults.
#include <cmath>

#include "abi_ctx.hpp"

extern "C" {

int32_t ssf_voxel_grid_batch(ssf_ctx* c, void* stream, int32_t n_clouds, const float* d_xyzi,
                             const int64_t* d_off, const int64_t* h_off, float leaf,
                             float* d_out, int32_t* d_out_count) {
    if (!c) return SSF_E_ARG;
    if (n_clouds < 0 || !(leaf > 0.0f) ||
        (n_clouds > 0 && (!d_xyzi || !d_off || !h_off || !d_out || !d_out_count)))
        return fail(c, SSF_E_ARG, "voxel_grid_batch: bad arguments");
    if (n_clouds == 0) return SSF_OK;
    int64_t max_pts = 0;
    for (int k = 0; k < n_clouds; ++k) {
        const int64_t m = h_off[k + 1] - h_off[k];
        if (m < 0) return fail(c, SSF_E_ARG, "voxel_grid_batch: offsets not monotone");
        if (m > (int64_t)INT32_MAX) return fail(c, SSF_E_ARG, "voxel_grid_batch: cloud too large");
        max_pts = std::max(max_pts, m);
    }
    if (h_off[0] != 0) return fail(c, SSF_E_ARG, "voxel_grid_batch: offsets must start at 0");
    const int64_t n = h_off[n_clouds];
    if (n > (int64_t)INT32_MAX) return fail(c, SSF_E_ARG, "voxel_grid_batch: too many points");
    hipStream_t s = (hipStream_t)stream;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    SSF_TRY_HIP(c, c->vg.ensure(ssf::vg_scratch_bytes(n_clouds, n)), "alloc voxel scratch");
    return hip_rc(c, ssf::launch_voxel_grid(s, n_clouds, reinterpret_cast<const float4*>(d_xyzi), d_off, n,
                                          max_pts, leaf, c->vg.p, reinterpret_cast<float4*>(d_out),
                                          d_out_count), "voxel_grid launch");
}

int32_t ssf_transform_clouds_batch(ssf_ctx* c, void* stream, int32_t n_clouds, const float* d_xyzi,
                                   const int64_t* d_off, const int64_t* h_off, const double* d_T,
                                   float* d_out) {
    if (!c) return SSF_E_ARG;
    if (n_clouds < 0 || (n_clouds > 0 && (!d_xyzi || !d_off || !h_off || !d_T || !d_out)))
        return fail(c, SSF_E_ARG, "transform_clouds_batch: bad arguments");
    if (n_clouds == 0) return SSF_OK;
    if (d_out == d_xyzi) return fail(c, SSF_E_ARG, "transform_clouds_batch: the output aliases the input");
    for (int k = 0; k < n_clouds; ++k)
        if (h_off[k + 1] < h_off[k]) return fail(c, SSF_E_ARG, "transform_clouds_batch: offsets not monotone");
    if (h_off[0] < 0) return fail(c, SSF_E_ARG, "transform_clouds_batch: negative offset");
    const int64_t total = h_off[n_clouds] - h_off[0];
    if (total == 0) return SSF_OK;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(c, stream);
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    return hip_rc(c, ssf::launch_transform_clouds(s, n_clouds, reinterpret_cast<const float4*>(d_xyzi), d_off,
                                                h_off[0], total, d_T, reinterpret_cast<float4*>(d_out)), "transform_clouds launch");
}

int32_t ssf_sc_params_default(ssf_sc_params* out) {
    if (!out) return SSF_E_ARG;
    out->max_range = 80.0f;
    out->lidar_height = 2.0f;
    out->threshold = 0.13f;
    return SSF_OK;
}

int32_t ssf_scan_context_batch(ssf_ctx* c, void* stream, int32_t n_clouds, const float* d_pts,
                               int32_t point_stride, const int64_t* d_off, const int64_t* h_off,
                               const ssf_sc_params* params, float* d_desc) {
    if (!c) return SSF_E_ARG;
    if (n_clouds < 0 || point_stride < 3 || point_stride > 4 || !params)
        return fail(c, SSF_E_ARG, "scan_context_batch: bad arguments (n_clouds >= 0, stride 3 or 4, params)");
    if (!std::isfinite(params->max_range) || !(params->max_range > 0.0f) || !std::isfinite(params->lidar_height))
        return fail(c, SSF_E_ARG, "scan_context_batch: max_range must be finite and positive, lidar_height finite");
    if (n_clouds > 0 && (!d_off || !h_off || !d_desc)) return fail(c, SSF_E_ARG, "scan_context_batch: null pointer");
    if (n_clouds == 0) return SSF_OK;
    for (int k = 0; k < n_clouds; ++k)
        if (h_off[k] < 0 || h_off[k + 1] < h_off[k])
            return fail(c, SSF_E_ARG, "scan_context_batch: offsets not monotone");
    if (!d_pts && h_off[n_clouds] != h_off[0])       // a batch of empty clouds has no points
        return fail(c, SSF_E_ARG, "scan_context_batch: null pointer");
    hipStream_t s = (hipStream_t)stream;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    ProfScope prof(c, stream);
    return hip_rc(c, ssf::launch_sc_describe(s, n_clouds, d_pts, point_stride, d_off, params->max_range,
                                           params->lidar_height, d_desc), "scan_context launch");
}

// Both matchers (who: the entry point's name in the messages): k == 0 selects each query's best
// candidate (launch_sc_match), k >= 1 its k best outside the exclusion window.
static int32_t sc_match(ssf_ctx* c, const std::string& who, void* stream, int32_t n_query,
                        const float* d_query, int32_t n_db, const float* d_db, const int32_t* d_n_eligible,
                        const int32_t* h_n_eligible, float* d_dist, int32_t* d_shift, ssf_sc_best* d_best,
                        int32_t k, int32_t exclusion) {
    if (n_query < 0 || n_db < 0) return fail(c, SSF_E_ARG, who + ": negative count");
    if ((d_dist == nullptr) != (d_shift == nullptr))
        return fail(c, SSF_E_ARG, who + ": d_dist and d_shift are given or null together");
    if (n_query > 0 && (!d_query || !d_n_eligible || !h_n_eligible || !d_best || (n_db > 0 && !d_db)))
        return fail(c, SSF_E_ARG, who + ": null pointer");
    if (n_query == 0) return SSF_OK;
    int32_t max_el = 0;
    for (int q = 0; q < n_query; ++q) {
        if (h_n_eligible[q] < 0 || h_n_eligible[q] > n_db)
            return fail(c, SSF_E_ARG, who + ": n_eligible outside 0 .. n_db");
        max_el = std::max(max_el, h_n_eligible[q]);
    }
    const int n_cols = d_dist ? n_db : max_el;
    if ((int64_t)n_query * ((n_cols + 15) / 16) >= ((int64_t)1 << 31))
        return fail(c, SSF_E_ARG, who + ": too many pairs for one call");
    hipStream_t s = (hipStream_t)stream;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    float* dist = d_dist;
    int32_t* shift = d_shift;
    if (!dist && n_cols > 0) {
        const size_t rows = (size_t)n_query * (size_t)n_db;
        SSF_TRY_HIP(c, c->sc_rows.ensure(rows * (sizeof(float) + sizeof(int32_t))), "alloc scan context rows");
        dist = c->sc_rows.as<float>();
        shift = reinterpret_cast<int32_t*>(dist + rows);
    }
    ProfScope prof(c, stream);
    return hip_rc(c, k == 0 ? ssf::launch_sc_match(s, n_query, d_query, n_db, n_cols, d_db, d_n_eligible, dist, shift, d_best)
                            : ssf::launch_sc_match_topk(s, n_query, d_query, n_db, n_cols, d_db, d_n_eligible, dist, shift,
                                                        k, exclusion, d_best),
                  (who + " launch").c_str());
}

int32_t ssf_scan_context_match(ssf_ctx* c, void* stream, int32_t n_query, const float* d_query,
                               int32_t n_db, const float* d_db, const int32_t* d_n_eligible,
                               const int32_t* h_n_eligible, float* d_dist, int32_t* d_shift,
                               ssf_sc_best* d_best) {
    if (!c) return SSF_E_ARG;
    return sc_match(c, "scan_context_match", stream, n_query, d_query, n_db, d_db, d_n_eligible, h_n_eligible,
                    d_dist, d_shift, d_best, 0, 0);
}

int32_t ssf_scan_context_match_topk(ssf_ctx* c, void* stream, int32_t n_query, const float* d_query,
                                    int32_t n_db, const float* d_db, const int32_t* d_n_eligible,
                                    const int32_t* h_n_eligible, float* d_dist, int32_t* d_shift,
                                    ssf_sc_best* d_best, int32_t k, int32_t exclusion) {
    if (!c) return SSF_E_ARG;
    if (k < 1 || k > SSF_SC_MAX_TOPK)
        return fail(c, SSF_E_ARG, "scan_context_match_topk: k outside 1 .. SSF_SC_MAX_TOPK");
    if (exclusion < 0) return fail(c, SSF_E_ARG, "scan_context_match_topk: negative exclusion");
    return sc_match(c, "scan_context_match_topk", stream, n_query, d_query, n_db, d_db, d_n_eligible,
                    h_n_eligible, d_dist, d_shift, d_best, k, exclusion);
}

int32_t ssf_icp_params_default(ssf_icp_params* out) {
    if (!out) return SSF_E_ARG;
    out->max_iter = 100;            // mapOptmization.cpp:225-228
    out->max_corr_dist = 50.0f;
    out->trans_eps = 1e-6;
    out->fit_eps = 1e-6;
    return SSF_OK;
}

int32_t ssf_icp_batch(ssf_ctx* c, void* stream, int32_t n_prob, const float* d_src,
                      const int64_t* d_src_off, const int64_t* h_src_off, const float* d_tgt,
                      const int64_t* d_tgt_off, const int64_t* h_tgt_off,
                      const ssf_icp_params* prm, const float* h_guess, double* h_out) {
    if (!c) return SSF_E_ARG;
    if (n_prob < 0 || !prm || prm->max_iter < 0 || !(prm->max_corr_dist >= 0.0f) ||
        (n_prob > 0 && (!d_src || !d_src_off || !h_src_off || !d_tgt || !d_tgt_off || !h_tgt_off || !h_out)))
        return fail(c, SSF_E_ARG, "icp_batch: bad arguments");
    if (n_prob == 0) return SSF_OK;
    int64_t max_ns = 0, max_nt = 0;
    for (int k = 0; k < n_prob; ++k) {
        const int64_t a = h_src_off[k + 1] - h_src_off[k], b = h_tgt_off[k + 1] - h_tgt_off[k];
        if (a < 0 || b < 0) return fail(c, SSF_E_ARG, "icp_batch: offsets not monotone");
        if (b > (int64_t)INT32_MAX) return fail(c, SSF_E_ARG, "icp_batch: target too large");
        max_ns = std::max(max_ns, a); max_nt = std::max(max_nt, b);
    }
    hipStream_t s = (hipStream_t)stream;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    SSF_TRY_HIP(c, c->icp_cur.ensure(sizeof(float4) * (size_t)std::max<int64_t>(h_src_off[n_prob], 1)), "alloc icp");
    SSF_TRY_HIP(c, c->icp_key.ensure(sizeof(unsigned long long) * (size_t)std::max<int64_t>(h_src_off[n_prob], 1)), "alloc icp");
    SSF_TRY_HIP(c, c->icp_st.ensure(sizeof(ssf::IcpState) * (size_t)n_prob), "alloc icp");
    SSF_TRY_HIP(c, c->icp_guess.ensure(sizeof(float) * 16 * (size_t)n_prob), "alloc icp");
    std::vector<float> g(16 * (size_t)n_prob, 0.0f);
    for (int k = 0; k < n_prob; ++k)
        for (int i = 0; i < 16; ++i) g[16 * k + i] = h_guess ? h_guess[16 * k + i] : (i % 5 == 0 ? 1.0f : 0.0f);
    SSF_TRY_HIP(c, hipMemcpyAsync(c->icp_guess.p, g.data(), sizeof(float) * g.size(), hipMemcpyHostToDevice, s), "H2D guess");
    const float4* src = reinterpret_cast<const float4*>(d_src);
    const float4* tgt = reinterpret_cast<const float4*>(d_tgt);
    float4* cur = c->icp_cur.as<float4>();
    unsigned long long* key = c->icp_key.as<unsigned long long>();
    ssf::IcpState* st = c->icp_st.as<ssf::IcpState>();
    SSF_TRY_HIP(c, ssf::launch_icp_init(s, n_prob, src, d_src_off, max_ns, c->icp_guess.as<float>(), cur, st, key), "icp init");
    // the iteration loop runs on device: every launch is skipped by problems already done; the
    // host polls the done flags every 8 iterations and stops once all problems have converged
    std::vector<ssf::IcpState> hs((size_t)n_prob);
    for (int it = 0; it < prm->max_iter; ++it) {
        SSF_TRY_HIP(c, ssf::launch_icp_iteration(s, n_prob, cur, d_src_off, max_ns, tgt, d_tgt_off, max_nt, *prm, st, key),
                    "icp iteration");
        if ((it & 7) == 7 || it + 1 == prm->max_iter) {
            SSF_TRY_HIP(c, hipMemcpyAsync(hs.data(), st, sizeof(ssf::IcpState) * hs.size(), hipMemcpyDeviceToHost, s), "D2H icp state");
            SSF_TRY_HIP(c, hipStreamSynchronize(s), "icp sync");
            bool all = true;
            for (const auto& x : hs) all = all && x.done;
            if (all) break;
        }
    }
    SSF_TRY_HIP(c, ssf::launch_icp_fitness(s, n_prob, src, d_src_off, h_src_off[n_prob], max_ns, tgt, d_tgt_off, max_nt, st, key),
                "icp fitness");
    SSF_TRY_HIP(c, hipMemcpyAsync(hs.data(), st, sizeof(ssf::IcpState) * hs.size(), hipMemcpyDeviceToHost, s), "D2H icp state");
    SSF_TRY_HIP(c, hipStreamSynchronize(s), "icp sync");
    for (int k = 0; k < n_prob; ++k) {
        double* o = h_out + (size_t)k * SSF_ICP_OUT_STRIDE;
        for (int i = 0; i < SSF_ICP_OUT_STRIDE; ++i) o[i] = 0.0;
        for (int i = 0; i < 16; ++i) o[SSF_ICP_OUT_T + i] = hs[k].fin[i];
        o[SSF_ICP_OUT_FITNESS] = hs[k].fitness;
        o[SSF_ICP_OUT_CONVERGED] = hs[k].converged;
        o[SSF_ICP_OUT_ITERATIONS] = hs[k].it;
        o[SSF_ICP_OUT_STATE] = hs[k].state;
        o[SSF_ICP_OUT_NCORR] = hs[k].n_corr;
    }
    return SSF_OK;
}

int32_t ssf_pgo_params_default(ssf_pgo_params* out) {
    if (!out) return SSF_E_ARG;
    out->max_iter = 8;              // mapOptmization.cpp:281-288: isam->update calls of a loop closure
    out->func_tol = 1e-6;           // the front-end's Ceres function tolerance
    return SSF_OK;
}

int32_t ssf_pgo_robust_default(int32_t kind, ssf_pgo_robust* out) {
    if (!out) return SSF_E_ARG;
    double k;                       // GTSAM's defaults (noiseModel::mEstimator)
    switch (kind) {
        case SSF_PGO_ROBUST_NONE: k = 0.0; break;
        case SSF_PGO_ROBUST_HUBER: k = 1.345; break;
        case SSF_PGO_ROBUST_CAUCHY: k = 0.1; break;
        case SSF_PGO_ROBUST_GEMAN_MCCLURE: k = 1.0; break;
        default: return SSF_E_ARG;
    }
    out->kind = kind;
    out->k = k;
    return SSF_OK;
}

// the pose-graph entry points; robust: the loss kernels and the per-edge output; lm: step control
static int32_t pose_graph_batch(ssf_ctx* c, void* stream, int32_t n_graphs, double* d_pose,
                                const int32_t* d_node_off, const int32_t* h_node_off,
                                const int32_t* d_edge_ij, const double* d_edge_meas,
                                const double* d_edge_var, const int32_t* d_edge_off,
                                const int32_t* h_edge_off, const double* d_prior_pose,
                                const double* d_prior_var, const ssf_pgo_params* prm,
                                double* d_stats, double* d_cost_log, bool robust, int rkind, double rk,
                                double* d_edge_out, const ssf_pgo_lm* lm, double* d_lm_log) {
    if (!c) return SSF_E_ARG;
    if (n_graphs < 0 || !prm || prm->max_iter < 0 || prm->max_iter > SSF_PGO_MAX_ITER ||
        !(prm->func_tol >= 0.0) ||
        (n_graphs > 0 && (!d_pose || !d_node_off || !h_node_off || !d_edge_ij || !d_edge_meas || !d_edge_var ||
                          !d_edge_off || !h_edge_off || !d_prior_pose || !d_prior_var || !d_stats)))
        return fail(c, SSF_E_ARG, "pose_graph_batch: bad arguments");
    if (n_graphs == 0) return SSF_OK;
    if (h_node_off[0] != 0 || h_edge_off[0] != 0)
        return fail(c, SSF_E_ARG, "pose_graph_batch: offsets must start at 0");
    for (int g = 0; g < n_graphs; ++g)
        if (h_node_off[g + 1] < h_node_off[g] || h_edge_off[g + 1] < h_edge_off[g])
            return fail(c, SSF_E_ARG, "pose_graph_batch: offsets not monotone");
    c->pgo_h.resize((size_t)n_graphs);
    size_t total = 0;
    bool any_narrow = false, any_wide = false;
    for (int g = 0; g < n_graphs; ++g) {
        ssf::PgoGraph& G = c->pgo_h[(size_t)g];
        G.node0 = h_node_off[g]; G.K = h_node_off[g + 1] - h_node_off[g];
        G.edge0 = h_edge_off[g]; G.E = h_edge_off[g + 1] - h_edge_off[g];
        G.lcap = std::min(std::max(G.E - (G.K - 1), 0), SSF_PGO_MAX_LOOPS);
        G.wide = ssf::pgo_graph_wide(G.K, G.E);
        (G.wide ? any_wide : any_narrow) = true;
        G.scratch_off = (int64_t)total;
        total += ssf::pgo_graph_doubles(G.K, G.E, G.lcap, G.wide != 0, lm != nullptr);
    }
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(c, stream);
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    SSF_TRY_HIP(c, c->pgo_desc.ensure(sizeof(ssf::PgoGraph) * (size_t)n_graphs), "alloc pose-graph descriptors");
    SSF_TRY_HIP(c, c->pgo_scratch.ensure(sizeof(double) * total), "alloc pose-graph scratch");
    SSF_TRY_HIP(c, hipMemcpyAsync(c->pgo_desc.p, c->pgo_h.data(), sizeof(ssf::PgoGraph) * (size_t)n_graphs,
                                  hipMemcpyHostToDevice, s), "H2D pose-graph descriptors");
    ssf::PgoArgs a{};
    a.desc = c->pgo_desc.as<ssf::PgoGraph>();
    a.pose = d_pose; a.node_off = d_node_off; a.edge_ij = d_edge_ij; a.edge_meas = d_edge_meas;
    a.edge_var = d_edge_var; a.edge_off = d_edge_off; a.prior_pose = d_prior_pose; a.prior_var = d_prior_var;
    a.max_iter = prm->max_iter; a.func_tol = prm->func_tol;
    a.scratch = c->pgo_scratch.as<double>();
    a.stats = d_stats; a.cost_log = d_cost_log;
    a.rkind = rkind; a.rk = rk; a.edge_out = d_edge_out;
    if (lm) a.lm = *lm;
    a.lm_log = d_lm_log;
    a.robust = robust; a.has_lm = lm != nullptr;
    return hip_rc(c, ssf::launch_pose_graph(s, n_graphs, any_narrow, any_wide, a), "pose_graph launch");
}

int32_t ssf_pose_graph_batch(ssf_ctx* c, void* stream, int32_t n_graphs, double* d_pose,
                             const int32_t* d_node_off, const int32_t* h_node_off,
                             const int32_t* d_edge_ij, const double* d_edge_meas,
                             const double* d_edge_var, const int32_t* d_edge_off,
                             const int32_t* h_edge_off, const double* d_prior_pose,
                             const double* d_prior_var, const ssf_pgo_params* prm,
                             double* d_stats, double* d_cost_log) {
    return pose_graph_batch(c, stream, n_graphs, d_pose, d_node_off, h_node_off, d_edge_ij, d_edge_meas,
                            d_edge_var, d_edge_off, h_edge_off, d_prior_pose, d_prior_var, prm, d_stats,
                            d_cost_log, false, SSF_PGO_ROBUST_NONE, 0.0, nullptr, nullptr, nullptr);
}

int32_t ssf_pose_graph_batch_robust(ssf_ctx* c, void* stream, int32_t n_graphs, double* d_pose,
                                    const int32_t* d_node_off, const int32_t* h_node_off,
                                    const int32_t* d_edge_ij, const double* d_edge_meas,
                                    const double* d_edge_var, const int32_t* d_edge_off,
                                    const int32_t* h_edge_off, const double* d_prior_pose,
                                    const double* d_prior_var, const ssf_pgo_params* prm,
                                    double* d_stats, double* d_cost_log, const ssf_pgo_robust* robust,
                                    double* d_edge_out) {
    return ssf_pose_graph_batch_lm(c, stream, n_graphs, d_pose, d_node_off, h_node_off, d_edge_ij, d_edge_meas,
                                   d_edge_var, d_edge_off, h_edge_off, d_prior_pose, d_prior_var, prm, d_stats,
                                   d_cost_log, robust, d_edge_out, nullptr, nullptr);
}

int32_t ssf_pgo_lm_default(ssf_pgo_lm* out) {
    if (!out) return SSF_E_ARG;
    out->radius0 = 1e4;             // Ceres' LevenbergMarquardtStrategy, as the front-end's solve
    out->min_relative_decrease = 1e-3;
    out->max_radius = 1e16;
    out->min_radius = 1e-32;
    return SSF_OK;
}

int32_t ssf_pose_graph_batch_lm(ssf_ctx* c, void* stream, int32_t n_graphs, double* d_pose,
                                const int32_t* d_node_off, const int32_t* h_node_off,
                                const int32_t* d_edge_ij, const double* d_edge_meas,
                                const double* d_edge_var, const int32_t* d_edge_off,
                                const int32_t* h_edge_off, const double* d_prior_pose,
                                const double* d_prior_var, const ssf_pgo_params* prm,
                                double* d_stats, double* d_cost_log, const ssf_pgo_robust* robust,
                                double* d_edge_out, const ssf_pgo_lm* lm, double* d_lm_log) {
    if (!c) return SSF_E_ARG;
    if (lm) {
        auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
        if (!pos(lm->radius0) || !pos(lm->max_radius) || !pos(lm->min_radius) || lm->min_radius > lm->max_radius)
            return fail(c, SSF_E_ARG, "pose_graph_batch_lm: radii must be finite, positive and min <= max");
        if (!(lm->min_relative_decrease >= 0.0 && lm->min_relative_decrease < 1.0))
            return fail(c, SSF_E_ARG, "pose_graph_batch_lm: min_relative_decrease must lie in [0, 1)");
    } else if (d_lm_log) {
        return fail(c, SSF_E_ARG, "pose_graph_batch_lm: d_lm_log needs lm");
    }
    const int rkind = robust ? robust->kind : SSF_PGO_ROBUST_NONE;
    if (rkind < SSF_PGO_ROBUST_NONE || rkind > SSF_PGO_ROBUST_GEMAN_MCCLURE)
        return fail(c, SSF_E_ARG, "pose_graph_batch_robust: unknown loss kind");
    if (rkind != SSF_PGO_ROBUST_NONE && !(std::isfinite(robust->k) && robust->k > 0.0))
        return fail(c, SSF_E_ARG, "pose_graph_batch_robust: k must be finite and positive");
    // no loss, no per-edge output and no step control: the plain kernels, launch for launch
    const bool plain = rkind == SSF_PGO_ROBUST_NONE && !d_edge_out && !lm;
    return pose_graph_batch(c, stream, n_graphs, d_pose, d_node_off, h_node_off, d_edge_ij, d_edge_meas,
                            d_edge_var, d_edge_off, h_edge_off, d_prior_pose, d_prior_var, prm, d_stats,
                            d_cost_log, !plain, rkind, rkind != SSF_PGO_ROBUST_NONE ? robust->k : 0.0,
                            d_edge_out, lm, d_lm_log);
}

}  // extern "C"
