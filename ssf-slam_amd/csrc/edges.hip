// edges.hip -- the point-to-line extension of the registration (beyond the reference, off by
// default): k_edge_table builds the last frames' line table, k_edge_associate the edge
// correspondence records; their blocks join k_solve<true, ..>'s evaluations (solve.hip).
#include "reg_knn.hpp"
#include "ssf_internal.hpp"

#include <algorithm>

namespace ssf {

// Edge features (beyond the reference; oracle/edge_oracle.c states the definitions).
// k_edge_table: one work-group per LAST frame, its edge cloud staged in LDS; per edge point the
// exact 5-NN (packed (distance, index) keys, brute force over the frame's few hundred edges),
// centroid + covariance in double in rank order, cyclic Jacobi, line test.
constexpr int kEdgeK = 5;
constexpr int kEdgeThreads = 1024;
constexpr int kEdgeLdsMax = 8192;          // edges per frame staged in LDS (128 KiB)

SSF_DEV void sym3_eig(double A[9], double V[9]) {       // = orc_sym3_eig, operation for operation
#pragma unroll
    for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = A[1] * A[1] + A[2] * A[2] + A[5] * A[5];
        const double dia = A[0] * A[0] + A[4] * A[4] + A[8] * A[8];
        if (!(off > 1e-30 * dia)) break;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int p = k == 2 ? 1 : 0, q = k == 0 ? 1 : 2;
            const double apq = A[3 * p + q];
            if (apq == 0.0) continue;
            const double theta = (A[3 * q + q] - A[3 * p + p]) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double aip = A[3 * i + p], aiq = A[3 * i + q];
                A[3 * i + p] = c * aip - sn * aiq;
                A[3 * i + q] = sn * aip + c * aiq;
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double api = A[3 * p + i], aqi = A[3 * q + i];
                A[3 * p + i] = c * api - sn * aqi;
                A[3 * q + i] = sn * api + c * aqi;
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double vip = V[3 * i + p], viq = V[3 * i + q];
                V[3 * i + p] = c * vip - sn * viq;
                V[3 * i + q] = sn * vip + c * viq;
            }
        }
    }
}

__global__ __launch_bounds__(kEdgeThreads) void k_edge_table(
    const float4* __restrict__ edges, const int64_t* __restrict__ frame_off,
    const int32_t* __restrict__ count, float max_nn_d2, float line_ratio, float* __restrict__ line,
    uint8_t* __restrict__ valid, int lds_cap) {
    extern __shared__ float4 EL[];
    const int f = blockIdx.x;
    const int m = count[f];
    const int64_t base = frame_off[f];
    const float4* E = edges + base;
    const bool in_lds = m <= lds_cap;                                   // uniform
    if (in_lds)
        for (int r = threadIdx.x; r < m; r += blockDim.x) EL[r] = E[r];
    __syncthreads();
    const float4* P = in_lds ? EL : E;
    for (int a = threadIdx.x; a < m; a += blockDim.x) {
        float* L = line + 6 * (base + a);
        float out[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        uint8_t ok = 0;
        if (m >= kEdgeK) {
            const float4 q = P[a];
            double kk[kEdgeK];
#pragma unroll
            for (int k = 0; k < kEdgeK; ++k) kk[k] = knn_key(__builtin_inff(), 0x7fffffff);
            for (int c = 0; c < m; ++c) {
                // most candidates of a brute-force scan are far: the insertion runs only when
                // some lane's candidate beats its 5th key (keys are exact, so order is kept)
                const double key = knn_key(l2_simple(q, P[c]), c);
                if (key < kk[kEdgeK - 1]) key_insert<kEdgeK>(kk, key);
            }
            double cen[3] = {0.0, 0.0, 0.0};
            float4 nb[kEdgeK];
#pragma unroll
            for (int k = 0; k < kEdgeK; ++k) {
                nb[k] = P[key_index(kk[k])];
                cen[0] += (double)nb[k].x; cen[1] += (double)nb[k].y; cen[2] += (double)nb[k].z;
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) cen[j] = cen[j] / 5.0;
            double A[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, V[9];
#pragma unroll
            for (int k = 0; k < kEdgeK; ++k) {
                const double v[3] = {(double)nb[k].x - cen[0], (double)nb[k].y - cen[1], (double)nb[k].z - cen[2]};
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) A[3 * r + c] += v[r] * v[c];
            }
#pragma unroll
            for (int j = 0; j < 9; ++j) A[j] = A[j] / 5.0;
            sym3_eig(A, V);
            const double w[3] = {A[0], A[4], A[8]};
            int i1 = 0;
            if (w[1] > w[i1]) i1 = 1;
            if (w[2] > w[i1]) i1 = 2;
            double l2 = -__builtin_inf();
#pragma unroll
            for (int i = 0; i < 3; ++i) if (i != i1 && w[i] > l2) l2 = w[i];
            double u[3] = {V[i1], V[3 + i1], V[6 + i1]};
            int big = 0;
            if (fabs(u[1]) > fabs(u[big])) big = 1;
            if (fabs(u[2]) > fabs(u[big])) big = 2;
            if (u[big] < 0.0) { u[0] = -u[0]; u[1] = -u[1]; u[2] = -u[2]; }
#pragma unroll
            for (int j = 0; j < 3; ++j) { out[j] = (float)cen[j]; out[3 + j] = (float)u[j]; }
            ok = (key_dist(kk[kEdgeK - 1]) < max_nn_d2) && (w[i1] > (double)line_ratio * l2) ? 1 : 0;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) L[j] = out[j];
        valid[base + a] = ok;
    }
}

// k_edge_associate: one work-group per pair.  Per current edge point, transformToLast (:74-82)
// and the exact 1-NN among the last frame's edges (brute force from LDS, (distance, index)
// order); the correspondence record carries the line (centroid in pa, direction in n) and its
// validity.  (A grid sized by the host's edge bound would launch ~50 mostly empty work-groups
// per pair, each holding the LDS staging size.)
constexpr int kEdgeAssocThreads = 1024;
__global__ __launch_bounds__(kEdgeAssocThreads) void k_edge_associate(
    const float4* __restrict__ last, const int64_t* __restrict__ last_off,
    const int32_t* __restrict__ last_count, const float* __restrict__ line,
    const uint8_t* __restrict__ line_valid, const float4* __restrict__ curr,
    const int64_t* __restrict__ curr_off, const int32_t* __restrict__ curr_count,
    const double* __restrict__ pose_rel, CorrRec* __restrict__ corr, int lds_cap) {
    extern __shared__ float4 LL[];
    const int p = blockIdx.x;
    const int mc = curr_count[p], ml = last_count[p];
    if (mc <= 0) return;                                                // uniform
    const int64_t lo = last_off[p], co = curr_off[p];
    const bool in_lds = ml <= lds_cap;                                  // uniform
    if (in_lds)
        for (int r = threadIdx.x; r < ml; r += blockDim.x) LL[r] = last[lo + r];
    __syncthreads();
    const float4* P = in_lds ? LL : last + lo;
    const double q[4] = {pose_rel[7 * p], pose_rel[7 * p + 1], pose_rel[7 * p + 2], pose_rel[7 * p + 3]};
    const double t[3] = {pose_rel[7 * p + 4], pose_rel[7 * p + 5], pose_rel[7 * p + 6]};
    for (int i = threadIdx.x; i < mc; i += blockDim.x) {
    const float4 pc = curr[co + i];
    const float4 qs = assoc_query_point(pc, q, t);
    float best = __builtin_inff();
    int bi = -1;
    for (int c = 0; c < ml; ++c) {
        const float d = l2_simple(qs, P[c]);
        if (d < best) { best = d; bi = c; }                             // ascending c: ties keep the lower index
    }
    CorrRec rec;
    rec.po[0] = pc.x; rec.po[1] = pc.y; rec.po[2] = pc.z;
    rec.valid = (bi >= 0 && line_valid[lo + bi]) ? 1.0f : 0.0f;
    // an empty last frame (bi < 0) has no row of its own: lo may be the table's row count
    float L[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (bi >= 0) {
        const float* row = line + 6 * (lo + bi);
#pragma unroll
        for (int j = 0; j < 6; ++j) L[j] = row[j];
    }
    rec.pa[0] = L[0]; rec.pa[1] = L[1]; rec.pa[2] = L[2]; rec.pad0 = 0.f;
    rec.n[0] = L[3]; rec.n[1] = L[4]; rec.n[2] = L[5]; rec.pad1 = 0.f;
    corr[co + i] = rec;
    }
}

// The edge association launch of launch_register (edge->max_m > 0).
void launch_edge_associate(hipStream_t s, int n_pairs, const EdgeReg* edge, const double* pin) {
    const int cap = (int)std::min<int64_t>(edge->max_m, kEdgeLdsMax);
    kmark(s, "k_edge_associate");
    hipLaunchKernelGGL(k_edge_associate, dim3(n_pairs), dim3(kEdgeAssocThreads), (size_t)cap * sizeof(float4),
                       s, edge->last, edge->last_off, edge->last_count, edge->line,
                       edge->line_valid, edge->curr, edge->curr_off, edge->curr_count, pin,
                       edge->corr, cap);
}

hipError_t launch_edge_table(hipStream_t s, const ssf_edge_config& ec, int n_frames,
                             const float4* edges, const int64_t* frame_off, const int32_t* count,
                             int64_t max_m, float* line, uint8_t* valid) {
    if (n_frames <= 0 || max_m <= 0) return hipSuccess;
    const int cap = (int)std::min<int64_t>(max_m, kEdgeLdsMax);
    kmark(s, "k_edge_table");
    hipLaunchKernelGGL(k_edge_table, dim3(n_frames), dim3(kEdgeThreads), (size_t)cap * sizeof(float4),
                       s, edges, frame_off, count, ec.max_nn_d2, ec.line_ratio, line, valid, cap);
    return hipGetLastError();
}

}  // namespace ssf
