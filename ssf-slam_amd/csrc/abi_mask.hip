// abi_mask.hip -- the scene-flow side's entry points: the dynamic-point mask + Kabsch pose on
// either storage, the float32 Kabsch tail and the seeded subsample.
#include <cstring>

#include "abi_ctx.hpp"

template <class T>
static int32_t mask_pose_batch(ssf_ctx* c, void* stream, int32_t n_frames, const T* d_pts,
                            const T* d_flow, const int64_t* d_frame_off,
                            const int64_t* h_frame_off, int32_t mode, const uint8_t* d_mask_in,
                            const double* h_draws, int32_t reflection, uint8_t* d_bg_mask,
                            double* d_out) {
    if (!c) return SSF_E_ARG;
    if (n_frames < 0 || mode < SSF_MASK_GMM || mode > SSF_MASK_GIVEN ||
        (n_frames > 0 && (!d_pts || !d_flow || !d_frame_off || !h_frame_off || !d_out)) ||
        (mode != SSF_MASK_GMM && !d_mask_in))
        return fail(c, SSF_E_ARG, "mask_pose_batch: bad arguments");
    if (n_frames == 0) return SSF_OK;
    if (c->mask_order && c->mask_order_n != n_frames)
        return fail(c, SSF_E_ARG, "mask_pose_batch: the frame order (ssf_set_mask_schedule) has another length");
    const int64_t total = h_frame_off[n_frames];
    for (int f = 0; f < n_frames; ++f) {
        if (h_frame_off[f + 1] < h_frame_off[f]) return fail(c, SSF_E_ARG, "mask_pose_batch: offsets not monotone");
        // the streaming loops address a frame with 32-bit byte offsets (mask_common.hpp load3_off)
        if (h_frame_off[f + 1] - h_frame_off[f] > (int64_t)(0xFFFFFFFFu / (3 * sizeof(T))))
            return fail(c, SSF_E_ARG, "mask_pose_batch: a frame above 2^32 / (3 sizeof(T)) points");
    }
    hipStream_t s = (hipStream_t)stream;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    ssf_ctx::DrawSlot& ds = c->dslot[c->dnext];
    c->dnext = (c->dnext + 1) % ssf_ctx::kDrawSlots;
    const size_t need = 3 * (size_t)n_frames;
    if (!ds.copied) {
        SSF_TRY_HIP(c, hipEventCreateWithFlags(&ds.copied, hipEventDisableTiming), "draws event");
        SSF_TRY_HIP(c, hipEventCreateWithFlags(&ds.used, hipEventDisableTiming), "draws event");
    } else {
        SSF_TRY_HIP(c, hipEventSynchronize(ds.copied), "draws event");   // staging reusable
    }
    const ssf::MaskPlan plan = ssf::mask_plan(n_frames, total, mode, c->mask_split, c->slots(), c->mask_queue);
    if (ds.d.bytes < plan.draws_bytes || ds.rec.bytes < plan.rec_bytes || ds.sync.bytes < plan.sync_bytes ||
        ds.parts.bytes < plan.parts_bytes) {                              // growing frees the old buffer
        SSF_TRY_HIP(c, hipEventSynchronize(ds.used), "draws event");
        SSF_TRY_HIP(c, ds.d.ensure(plan.draws_bytes), "alloc draws");
        if (plan.rec_bytes) SSF_TRY_HIP(c, ds.rec.ensure(plan.rec_bytes), "alloc lloyd records");
        if (plan.sync_bytes) SSF_TRY_HIP(c, ds.sync.ensure(plan.sync_bytes), "alloc mask sync");
        if (plan.parts_bytes) SSF_TRY_HIP(c, ds.parts.ensure(plan.parts_bytes), "alloc mask parts");
    } else {
        SSF_TRY_HIP(c, hipStreamWaitEvent(s, ds.used, 0), "draws wait");   // device-side: no host stall
    }
    if (ds.hcap < (int64_t)need) {
        if (ds.h) SSF_TRY_HIP(c, hipHostFree(ds.h), "free pinned");
        ds.h = nullptr; ds.hcap = 0;
        SSF_TRY_HIP(c, hipHostMalloc((void**)&ds.h, sizeof(double) * need), "pinned draws");
        ds.hcap = (int64_t)need;
    }
    std::memset(ds.h, 0, sizeof(double) * need);
    if (mode == SSF_MASK_GMM) {
        for (int f = 0; f < n_frames; ++f) {
            const int64_t nf = h_frame_off[f + 1] - h_frame_off[f];
            double u0, u1, u2;
            if (h_draws) { u0 = h_draws[3 * f]; u1 = h_draws[3 * f + 1]; u2 = h_draws[3 * f + 2]; }
            else { u0 = c->rng.random_sample(); u1 = c->rng.random_sample(); u2 = c->rng.random_sample(); }
            ds.h[3 * f] = nf > 0 ? (double)c->rng.choice_uniform(nf, u0) : 0.0;
            ds.h[3 * f + 1] = u1;
            ds.h[3 * f + 2] = u2;
        }
    }
    SSF_TRY_HIP(c, hipMemcpyAsync(ds.d.p, ds.h, sizeof(double) * need, hipMemcpyHostToDevice, s), "H2D draws");
    SSF_TRY_HIP(c, hipEventRecord(ds.copied, s), "draws record");
    ProfScope prof(c, stream);
    ssf::MaskArgs<T> a{};
    a.pts = d_pts; a.flow = d_flow; a.frame_off = d_frame_off;
    a.mode = mode; a.mask_in = d_mask_in;
    a.draws = ds.d.as<double>(); a.lloyd_rec = ds.rec.as<uint2>();
    a.reflection = reflection; a.bg_mask = d_bg_mask; a.out = d_out;
    a.sync = ds.sync.as<uint32_t>(); a.parts = ds.parts.as<double>();
    a.order = c->mask_order;
    hipError_t e = ssf::launch_mask_pose(s, n_frames, plan, a);
    if (e == hipSuccess) e = hipEventRecord(ds.used, s);
    if (e != hipSuccess) return hip_fail(c, e, "mask_pose launch");
    return SSF_OK;
}

extern "C" {

int32_t ssf_mask_pose_batch(ssf_ctx* c, void* stream, int32_t n_frames, const float* d_pts,
                            const float* d_flow, const int64_t* d_frame_off,
                            const int64_t* h_frame_off, int32_t mode, const uint8_t* d_mask_in,
                            const double* h_draws, int32_t reflection, uint8_t* d_bg_mask,
                            double* d_out) {
    return mask_pose_batch(c, stream, n_frames, d_pts, d_flow, d_frame_off, h_frame_off, mode,
                           d_mask_in, h_draws, reflection, d_bg_mask, d_out);
}

int32_t ssf_mask_pose_batch_f64(ssf_ctx* c, void* stream, int32_t n_frames, const double* d_pts,
                                const double* d_flow, const int64_t* d_frame_off,
                                const int64_t* h_frame_off, int32_t mode, const uint8_t* d_mask_in,
                                const double* h_draws, int32_t reflection, uint8_t* d_bg_mask,
                                double* d_out) {
    return mask_pose_batch(c, stream, n_frames, d_pts, d_flow, d_frame_off, h_frame_off, mode,
                           d_mask_in, h_draws, reflection, d_bg_mask, d_out);
}

int32_t ssf_kabsch_f32_batch(ssf_ctx* c, void* stream, int32_t n_frames, const float* d_src,
                             const float* d_dst, const float* d_flow, const int64_t* d_frame_off,
                             const uint8_t* d_mask, int32_t reflection, int32_t after_mask,
                             double* d_out) {
    if (!c) return SSF_E_ARG;
    if (n_frames < 0 || (n_frames > 0 && (!d_dst || (!d_flow && !d_src) || !d_frame_off || !d_out)))
        return fail(c, SSF_E_ARG, "kabsch_f32_batch: bad arguments");
    if (n_frames == 0) return SSF_OK;
    hipStream_t s = (hipStream_t)stream;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    ProfScope prof(c, stream);
    return hip_rc(c, ssf::launch_kabsch_f32(s, n_frames, d_src, d_dst, d_flow, d_frame_off, d_mask,
                                          reflection ? 1 : 0, after_mask ? 1 : 0, d_out), "kabsch_f32 launch");
}

int32_t ssf_subsample_batch(ssf_ctx* c, void* stream, int32_t n_frames, const float* d_pts,
                            int32_t point_stride, const int64_t* d_frame_off,
                            const int64_t* h_frame_off, const uint8_t* d_class, int32_t nb,
                            float z_min, int32_t use_z, int32_t quota, uint64_t seed,
                            const uint64_t* h_tag, int32_t key_bits, int32_t* d_idx, float* d_xyz,
                            int32_t* d_n, int32_t* d_status) {
    if (!c) return SSF_E_ARG;
    if (n_frames < 0 || nb < 1 || nb > SSF_SAMPLE_MAX_NB || point_stride < 3 || key_bits < 1 ||
        key_bits > 32 || quota < -1 || (quota >= 0 && !d_class))
        return fail(c, SSF_E_ARG, "subsample_batch: bad arguments (1 <= nb <= 8192, stride >= 3, "
                                  "1 <= key_bits <= 32, quota >= -1 and a class array with a quota)");
    if (n_frames > 0 && (!d_frame_off || !h_frame_off || !d_idx || !d_n || !d_status))
        return fail(c, SSF_E_ARG, "subsample_batch: null pointer");
    if (n_frames == 0) return SSF_OK;
    if (!d_pts && h_frame_off[n_frames] != h_frame_off[0])      // a batch of empty frames has no points
        return fail(c, SSF_E_ARG, "subsample_batch: null pointer");
    for (int k = 0; k < n_frames; ++k) {
        const int64_t m = h_frame_off[k + 1] - h_frame_off[k];
        if (m < 0 || h_frame_off[k] < 0) return fail(c, SSF_E_ARG, "subsample_batch: offsets not monotone");
        if (m > (int64_t)SSF_SAMPLE_MAX_POINTS)
            return fail(c, SSF_E_ARG, "subsample_batch: a frame holds more than 2^24 points");
    }
    hipStream_t s = (hipStream_t)stream;
    SSF_TRY_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    ProfScope prof(c, stream);
    return hip_rc(c, ssf::launch_subsample(s, n_frames, d_pts, point_stride, d_frame_off, d_class, nb,
                                         z_min, use_z, quota, seed, h_tag, key_bits, d_idx, d_xyz,
                                         d_n, d_status), "subsample launch");
}

}  // extern "C"
