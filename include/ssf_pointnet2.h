/*
 * ssf_pointnet2.h -- C ABI of the point-set operators of the TFlow scene-flow network
 *  on MI355X (gfx950).
 *
 * The reference imports these operators as `lib.pointnet2_utils` (the "pointutils" module of
 * scripts/ActiveSceneFlow/utils/utils.py:7 and utils/soflow.py:7), a CUDA extension that is not
 * vendored in the repository.  Each entry point below replaces one of its functions, with the
 * semantics of the reference's own torch restatement of that operator (cited per function).
 *
 * Conventions
 *   - d_ pointers are DEVICE pointers owned by the caller; `stream` is a hipStream_t (NULL = the
 *     default stream).  Every call is asynchronous on `stream` and stateless (no context).
 *   - Coordinates are [B, N, 3] float32 (the extension's "xyz_t" layout) unless stated;
 *     features are [B, C, N] float32; indices are int32.
 *   - Return 0 on success, <0 on error; ssf_pn2_last_error() describes the calling thread's
 *     last error.  Indices outside their range read as 0 and set *d_bad (device int32) to 1.
 *
 * Entry point                     replaces (scripts/ActiveSceneFlow)
 *   ssf_pn2_furthest_point_sample pointutils.furthest_point_sample        utils/utils.py:226
 *   ssf_pn2_knn / _three_nn       pointutils.knn / three_nn               utils/utils.py:229,560
 *   ssf_pn2_gather                pointutils.gather_ / grouping_operation utils/utils.py:228,231
 *   ssf_pn2_group_relative        the grouping block of a set abstraction utils/utils.py:228-234
 *   ssf_pn2_three_interpolate     pointutils.three_interpolate            utils/utils.py:658-663
 *   ssf_pn2_upsample_flow         UpsampleFlow.forward                    utils/soflow.py:1442-1470
 *   ssf_pn2_grouped_mlp_max       grouping + mlp + max of PointNetSetAbstraction (utils.py:231-247)
 *                                 and of PointNetSetUpConv's mlp1 (utils.py:296-307), one kernel
 *   ssf_pn2_grouped_mlp           the grouped MLPs of PointConvTransFlowV2 (mlp_convs .. mlp_convs4,
 *                                 weightnet1)                              utils/soflow.py:392-509
 *   ssf_pn2_pair_attention        the k x k mutual attention of a cost volume utils/soflow.py:420-458
 *   ssf_pn2_segment_softmax_sum   softmax-weighted sums, by centroid or by scatter target
 *                                 (torch_scatter's scatter_softmax, scatter_sum) utils/soflow.py:469-486
 */
#ifndef SSF_POINTNET2_H
#define SSF_POINTNET2_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SSF_PN2_OK 0
#define SSF_PN2_E_ARG (-1)
#define SSF_PN2_E_HIP (-2)
#define SSF_PN2_KNN_MAX 32
#define SSF_PN2_UPSAMPLE_MAX_SPARSE 4096
#define SSF_PN2_MLP_MAX_LAYERS 3
#define SSF_PN2_MLP_MAX_WIDTH 512
#define SSF_PN2_GMLP_MAX_IN 766
#define SSF_PN2_ATTN_MAX_C 512

const char* ssf_pn2_last_error(void);

/* pointutils.furthest_point_sample(xyz_t, npoint) (utils/utils.py:226; torch restatement
 * farthest_point_sample, :68-89): d_xyz [b, n, 3] -> d_idx [b, npoint].  The first centroid is
 * d_start[i] (nullable = 0, the extension's choice; the torch restatement draws it with
 * torch.randint).  Squared distances in f32 ((dx^2 + dy^2) + dz^2), running minimum, argmax with
 * ties to the lowest index (torch.max).  d_temp: b * n floats of scratch, needed when n > 16384
 * (nullable otherwise). */
int32_t ssf_pn2_furthest_point_sample(void* stream, int32_t b, int32_t n, int32_t npoint,
                                      const float* d_xyz, const int32_t* d_start, float* d_temp,
                                      int32_t* d_idx);

/* pointutils.knn(k, query, ref) (utils/utils.py:229,291,397,604; soflow.py:1461; torch
 * restatement knn_point, :92-108): for each of the s_q points of d_query [b, s_q, 3], the k
 * (<= 32) nearest of the n points of d_ref [b, n, 3], ascending by f32 squared distance, ties
 * to the lower index.  d_dist [b, s_q, k] = sqrt(squared distance) (:108), d_idx [b, s_q, k]. */
int32_t ssf_pn2_knn(void* stream, int32_t b, int32_t s_q, int32_t n, int32_t k,
                    const float* d_query, const float* d_ref, float* d_dist, int32_t* d_idx);

/* pointutils.three_nn(unknown, known) (utils/utils.py:560,658; soflow.py:1459): knn with k = 3,
 * d_dist / d_idx [b, n, 3]. */
int32_t ssf_pn2_three_nn(void* stream, int32_t b, int32_t n, int32_t m, const float* d_unknown,
                         const float* d_known, float* d_dist, int32_t* d_idx);

/* pointutils.gather_operation(features, idx) (utils/utils.py:228) with g = S indices per batch
 * element ([b, c, n] x [b, g] -> [b, c, g]), and pointutils.grouping_operation(features, idx)
 * (:231,233; soflow.py:30,1462,1472) with g = S * K ([b, c, n] x [b, S, K] -> [b, c, S, K]).
 * Torch restatements: index_points (utils.py:48-65), index_points_group (soflow.py:21-32). */
int32_t ssf_pn2_gather(void* stream, int32_t b, int32_t c, int32_t n, int32_t g,
                       const float* d_feat, const int32_t* d_idx, float* d_out, int32_t* d_bad);

/* The grouping block of PointNetSetAbstraction.forward (utils/utils.py:228-234) in one call:
 * out [b, 3 + c, s, k] = cat(grouping(xyz, idx) - new_xyz[..., None], grouping(feat, idx)),
 * with d_xyz [b, 3, n] (n <= 36864), d_new_xyz [b, 3, s], d_feat [b, c, n] (nullable when
 * c = 0), d_idx [b, s, k]. */
int32_t ssf_pn2_group_relative(void* stream, int32_t b, int32_t n, int32_t s, int32_t k, int32_t c,
                               const float* d_xyz, const float* d_new_xyz, const float* d_feat,
                               const int32_t* d_idx, float* d_out, int32_t* d_bad);

/* The grouping block above, the shared mlp and the max over the k samples of
 * PointNetSetAbstraction.forward (utils/utils.py:231-247) in one kernel, with no [b, C, s, k]
 * tensor in memory.  Per centroid j and sample m the input column is
 * cat(xyz[:, idx[j, m]] - new_xyz[:, j], feat[:, idx[j, m]]) (3 + c channels, the order of
 * :232-234); layer l computes y[o] = max(0, fmaf(sum_i wt[i][o] x[i], scale[o], shift[o])) -- a
 * bias-free 1x1 convolution (sum over i ascending, an f32 fma chain), eval-mode BatchNorm folded
 * into scale and shift by the caller, ReLU -- and d_out [b, widths[n_layers], s] is the max over
 * the k samples of the last layer.
 *   d_xyz [b, 3, n] (n <= 36864), d_new_xyz [b, 3, s], d_feat [b, c, n] (nullable when c = 0),
 *   d_idx [b, s, k] (1 <= k <= SSF_PN2_KNN_MAX);
 *   widths: HOST array of n_layers + 1 ints (1 <= n_layers <= SSF_PN2_MLP_MAX_LAYERS, every
 *   width in [1, SSF_PN2_MLP_MAX_WIDTH], widths[0] = 3 + c);
 *   d_wt / d_scale / d_shift: HOST arrays of n_layers DEVICE pointers; layer l's weights are
 *   [widths[l], widths[l + 1]] (input-major), its scale and shift [widths[l + 1]].
 * Writes exactly b * widths[n_layers] * s floats, allocates nothing, launches one kernel; a
 * batch element's output does not depend on the rest of the batch. */
int32_t ssf_pn2_grouped_mlp_max(void* stream, int32_t b, int32_t n, int32_t s, int32_t k, int32_t c,
                                const float* d_xyz, const float* d_new_xyz, const float* d_feat,
                                const int32_t* d_idx, int32_t n_layers, const int32_t* widths,
                                const float* const* d_wt, const float* const* d_scale,
                                const float* const* d_shift, float* d_out, int32_t* d_bad);

/* The grouped MLP above, generalised for the cost volume of PointConvTransFlowV2
 * (utils/soflow.py:392-509).  Per centroid j and sample m the input column is the concatenation,
 * in this order, of up to four segments (a segment with a null pointer / zero width is absent):
 *   1. d_ctr [b, c_ctr, s]:        ctr[:, j], one value per centroid, the same for every m;
 *   2. d_feat [b, c_g, n]:         feat[:, idx[j, m]];
 *   3. d_dense [b, c_d, s, k]:     dense[:, j, m];
 *   4. d_xyz [b, 3, n] with d_new_xyz [b, 3, s]:  xyz[:, idx[j, m]] - new_xyz[:, j] (3 channels).
 * Layer l computes t = fmaf(sum_i wt[i][o] x[i], scale[o], shift[o]) (i ascending, an f32 fma
 * chain) and y = t > 0 ? t : slope[l] * t: slope 0 is ReLU, 0.1 the reference's LeakyReLU, 1 no
 * activation.  A convolution bias is scale = 1, shift = bias.
 *   d_idx [b, s, k] is needed (with 0 < n <= 36864) when segment 2 or 4 is present, else nullable;
 *   widths: HOST array of n_layers + 1 ints, 1 <= n_layers <= SSF_PN2_MLP_MAX_LAYERS;
 *   widths[0] = c_ctr + c_g + c_d + (d_xyz ? 3 : 0), in [1, SSF_PN2_GMLP_MAX_IN]; every other
 *   width in [1, SSF_PN2_MLP_MAX_WIDTH].  766 input rows are what two LDS images of a 32-column
 *   tile leave beside a 512-row second image: (766 * 32 + 64 + 512 * 32) * 4 B = 160 KiB;
 *   d_wt / d_scale / d_shift: HOST arrays of n_layers DEVICE pointers, as for grouped_mlp_max;
 *   slope: HOST array of n_layers floats;  1 <= k <= SSF_PN2_KNN_MAX.
 * full_output = 0: d_out [b, widths[n_layers], s], the max over the k samples;
 * full_output = 1: d_out [b, widths[n_layers], s, k], every column.
 * Writes exactly that many floats, allocates nothing, launches one kernel; a batch element's
 * output does not depend on the rest of the batch and is the same from run to run. */
int32_t ssf_pn2_grouped_mlp(void* stream, int32_t b, int32_t n, int32_t s, int32_t k, int32_t c_ctr,
                            int32_t c_g, int32_t c_d, const float* d_ctr, const float* d_feat,
                            const float* d_dense, const float* d_xyz, const float* d_new_xyz,
                            const int32_t* d_idx, int32_t n_layers, const int32_t* widths,
                            const float* const* d_wt, const float* const* d_scale,
                            const float* const* d_shift, const float* slope, int32_t full_output,
                            float* d_out, int32_t* d_bad);

/* The mutual attention between the two grouped feature sets of a cost volume
 * (utils/soflow.py:420-458), one launch.  d_q, d_kw [b, c, s, k] -> d_qm, d_kwm [b, c, s, k].  Per
 * centroid: a[m][m'] = sum_ch q[ch][m] kw[ch][m'] (ch ascending, fma chain; no 1 / sqrt(c)),
 * W = softmax over m of a (times) softmax over m' of a, with expf on max-subtracted arguments,
 *   qm[ch][m]   = q[ch][m]   + sum_m' W[m][m'] kw[ch][m'],
 *   kwm[ch][m'] = kw[ch][m'] + sum_m  q[ch][m] W[m][m'],   both sums ascending.
 * 1 <= c <= SSF_PN2_ATTN_MAX_C, 1 <= k <= SSF_PN2_KNN_MAX.  The outputs must not alias the inputs. */
int32_t ssf_pn2_pair_attention(void* stream, int32_t b, int32_t c, int32_t s, int32_t k,
                               const float* d_q, const float* d_kw, float* d_qm, float* d_kwm);

/* Softmax-weighted sums over segments of a flat entry list (utils/soflow.py:469-486).
 * d_logit [b, m], d_val [b, c, m] -> d_out [b, c, t_n]:
 *   out[ch][t] = sum_e w_e val[ch][e],  w_e = expf(l_e - max_seg) / sum_seg expf(l - max_seg),
 * over the entries e of segment t, in the segment's order (fma chain); an empty segment gives 0.
 *   uniform segments: d_offsets = d_order = NULL and m = t_n * k: segment t = entries
 *     [t k, (t + 1) k) (weights1 and point_to_patch_cost_fwd, :469,:486);
 *   CSR segments: d_offsets [b, t_n + 1] (ascending, within [0, m]) and d_order [b, m], the entries
 *     grouped by segment (scatter_softmax, the product and scatter_sum of :474-481); k is ignored.
 * An entry of d_order outside [0, m) reads as entry 0, an offset outside [0, m] or below its
 * predecessor is clamped, and either sets *d_bad.  Segments may have any length. */
int32_t ssf_pn2_segment_softmax_sum(void* stream, int32_t b, int32_t c, int32_t m, int32_t t_n,
                                    int32_t k, const float* d_logit, const float* d_val,
                                    const int32_t* d_offsets, const int32_t* d_order, float* d_out,
                                    int32_t* d_bad);

/* pointutils.three_interpolate(features [b, c, m], idx [b, n, 3], weight [b, n, 3]) ->
 * [b, c, n]: w0 f[i0] + w1 f[i1] + w2 f[i2] (the weighted 3-NN sum of
 * PointNetFeaturePropogation, utils/utils.py:658-663). */
int32_t ssf_pn2_three_interpolate(void* stream, int32_t b, int32_t c, int32_t m, int32_t n,
                                  const float* d_feat, const int32_t* d_idx, const float* d_weight,
                                  float* d_out, int32_t* d_bad);

/* UpsampleFlow.forward(xyz, sparse_xyz, sparse_flow, k) (utils/soflow.py:1442-1470), fused:
 * d_xyz [b, 3, n], d_sparse_xyz [b, 3, s] (s <= 4096), d_sparse_feat [b, c, s] -> d_out
 * [b, c, n]: k (<= 16) nearest sparse points (three_nn for k = 3), inverse Euclidean distances
 * (clamped at 1e-10) normalised to sum 1, weighted feature sum clamped to [-100, 100]. */
int32_t ssf_pn2_upsample_flow(void* stream, int32_t b, int32_t n, int32_t s, int32_t c, int32_t k,
                              const float* d_xyz, const float* d_sparse_xyz,
                              const float* d_sparse_feat, float* d_out);

#ifdef __cplusplus
}
#endif
#endif
