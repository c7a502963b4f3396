// abi_core.hip -- the context's own entry points: version, configuration defaults, create /
// destroy, the last error, kernel timing, the setters, the RandomState seed and ssf_reserve.
#include <cstring>
#include <new>

#include "abi_ctx.hpp"

thread_local KTimer* KTimer::current = nullptr;

void ssf::kmark(hipStream_t s, const char* name) {
    if (KTimer::current) KTimer::current->mark(s, name);
}

static bool valid_cfg(const ssf_config& c) {
    return (c.n_rows == 16 || c.n_rows == 64) && c.plane_span >= 2 && c.row_start >= 0 &&
           c.row_end >= 0 && c.max_iter >= 0 && c.max_iter <= 64 &&
           (c.solver == SSF_SOLVER_CERES_LM || c.solver == SSF_SOLVER_GN) &&
           (c.ring_chain == SSF_RING_CHAIN_FLOAT || c.ring_chain == SSF_RING_CHAIN_DOUBLE);
}

extern "C" {

int32_t ssf_abi_version(void) { return SSF_ABI_VERSION; }

int32_t ssf_config_default(int32_t n_rows, ssf_config* out) {
    if (!out) return SSF_E_ARG;
    std::memset(out, 0, sizeof(*out));
    out->n_rows = n_rows;
    out->solver = SSF_SOLVER_CERES_LM;
    out->max_iter = 8;                          // lidarOdometry_onlyPC.cpp:246
    out->ring_chain = SSF_RING_CHAIN_FLOAT;     // frameFeature.cpp:57 under libstdc++
    if (n_rows == 16) {                         // frameFeature.cpp:143-146, onlyPC:314-316
        out->plane_min = 0.05f; out->plane_span = 3; out->plane_max = 0.15f;
        return SSF_OK;
    }
    if (n_rows == 64) {                         // frameFeature.cpp:147-152, onlyPC:317-319
        out->plane_min = 0.005f; out->plane_span = 25; out->row_start = 5; out->row_end = 5;
        out->plane_max = 0.05f;
        return SSF_OK;
    }
    return SSF_E_ARG;
}

int32_t ssf_create(int32_t device, const ssf_config* cfg, ssf_ctx** out) {
    if (!out || !cfg || !valid_cfg(*cfg)) return SSF_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return SSF_E_NODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return SSF_E_NODEV;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SSF_E_NODEV;
    ssf_ctx* c = new (std::nothrow) ssf_ctx();
    if (!c) return SSF_E_NOMEM;
    c->device = device;
    c->cfg = *cfg;
    ssf_edge_config_default(cfg->n_rows, &c->ecfg);
    *out = c;
    return SSF_OK;
}

void ssf_destroy(ssf_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (!c->prof.marks.empty()) (void)hipEventSynchronize(c->prof.marks.back().ev);
    delete c;                                   // the members release what they hold (abi_ctx.hpp)
}

int32_t ssf_profile_enable(ssf_ctx* c, int32_t on) {
    if (!c) return SSF_E_ARG;
    c->prof.on = on != 0;
    return SSF_OK;
}

int32_t ssf_profile_read(ssf_ctx* c, ssf_kernel_time* out, int32_t cap, int32_t* n_out) {
    if (!c || !n_out || cap < 0 || (cap > 0 && !out)) return SSF_E_ARG;
    *n_out = 0;
    KTimer& P = c->prof;
    if (P.marks.empty()) return SSF_OK;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    for (const auto& m : P.marks) SSF_TRY_HIP(c, hipEventSynchronize(m.ev), "profile sync");
    int n = 0;
    for (size_t i = 0; i + 1 < P.marks.size(); ++i) {
        const char* nm = P.marks[i].name;
        if (!nm) continue;                               // between two ABI calls: no kernel
        float ms = 0.0f;
        SSF_TRY_HIP(c, hipEventElapsedTime(&ms, P.marks[i].ev, P.marks[i + 1].ev), "profile elapsed");
        int k = 0;
        while (k < n && std::strncmp(out[k].name, nm, sizeof(out[k].name)) != 0) ++k;
        if (k == n) {
            if (n == cap) continue;
            std::memset(&out[k], 0, sizeof(out[k]));
            std::strncpy(out[k].name, nm, sizeof(out[k].name) - 1);
            ++n;
        }
        out[k].launches += 1;
        out[k].total_ms += ms;
    }
    P.marks.clear();
    *n_out = n;
    return SSF_OK;
}

const char* ssf_last_error(const ssf_ctx* c) { return c ? c->err.c_str() : "null context"; }

int32_t ssf_set_mask_schedule(ssf_ctx* c, const int32_t* d_order, int32_t n_order, int32_t queue) {
    if (!c) return SSF_E_ARG;
    if (queue < 0 || (d_order && n_order <= 0)) return fail(c, SSF_E_ARG, "set_mask_schedule: bad arguments");
    c->mask_order = d_order;
    c->mask_order_n = d_order ? n_order : 0;
    c->mask_queue = queue;
    return SSF_OK;
}

int32_t ssf_set_mask_split(ssf_ctx* c, int32_t parts_per_frame) {
    if (!c || parts_per_frame < 0 || parts_per_frame > ssf::kMaskMaxSplit) return SSF_E_ARG;
    c->mask_split = parts_per_frame;
    return SSF_OK;
}

int32_t ssf_edge_config_default(int32_t n_rows, ssf_edge_config* out) {
    if (!out || (n_rows != 16 && n_rows != 64)) return SSF_E_ARG;
    out->edge_min = 1.0f;
    out->edge_span = n_rows == 64 ? 10 : 3;
    out->line_ratio = 3.0f;
    out->max_nn_d2 = 1.0f;
    return SSF_OK;
}

int32_t ssf_set_edge_config(ssf_ctx* c, const ssf_edge_config* ec) {
    if (!c || !ec || ec->edge_span < 1 || !(ec->line_ratio >= 1.0f) || !(ec->max_nn_d2 > 0.0f))
        return c ? fail(c, SSF_E_ARG, "set_edge_config: bad arguments") : SSF_E_ARG;
    c->ecfg = *ec;
    return SSF_OK;
}

int32_t ssf_rng_seed(ssf_ctx* c, uint32_t seed) {
    if (!c) return SSF_E_ARG;
    c->rng.seed(seed);
    return SSF_OK;
}

// Every size here comes from the function that sizes the same buffer for a launch.
int32_t ssf_reserve(ssf_ctx* c, int32_t max_frames, int64_t max_points_per_frame) {
    if (!c || max_frames < 0 || max_points_per_frame < 0) return SSF_E_ARG;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    const int64_t total = (int64_t)max_frames * max_points_per_frame;
    int32_t rc = ensure_features(c, max_frames, total, max_points_per_frame);
    if (rc) return rc;
    SSF_TRY_HIP(c, c->corr.ensure(ssf::reg_corr_bytes(total)), "alloc corr");
    SSF_TRY_HIP(c, c->cidx.ensure(ssf::reg_cidx_bytes(total, max_frames)), "alloc corr index");
    // a GMM launch of max_frames frames under the automatic split (a fixed split grows its
    // exchange slots on demand), and its sync words also where a frame queue runs it instead
    const int nf = std::max(max_frames, 1);
    const ssf::MaskPlan split = ssf::mask_plan(nf, total, SSF_MASK_GMM, 0, c->slots(), 0);
    const ssf::MaskPlan queued = ssf::mask_plan(nf, total, SSF_MASK_GMM, 1, c->slots(), 1);
    for (auto& ds : c->dslot) {
        SSF_TRY_HIP(c, ds.d.ensure(split.draws_bytes), "alloc draws");
        SSF_TRY_HIP(c, ds.rec.ensure(split.rec_bytes), "alloc lloyd records");
        SSF_TRY_HIP(c, ds.sync.ensure(std::max(split.sync_bytes, queued.sync_bytes)), "alloc mask sync");
        if (split.parts_bytes) SSF_TRY_HIP(c, ds.parts.ensure(split.parts_bytes), "alloc mask parts");
    }
    return SSF_OK;
}

}  // extern "C"
