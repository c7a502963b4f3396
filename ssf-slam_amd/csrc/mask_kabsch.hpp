// mask_kabsch.hpp -- the Kabsch tail of k_mask_pose: the shifted per-point sums and, on one
// lane, the 3x3 SVD, R, t and the pyquaternion trace-method q.
#pragma once
#include "mask_common.hpp"
#include "svd3.hpp"

namespace ssf {

SSF_DEV void accum_kabsch(double (&k)[16], const double* x, const double cs[3], const double cd[3]) {
    double s[3], d[3];
    for (int i = 0; i < 3; ++i) { d[i] = x[3 + i] - cd[i]; s[i] = (x[3 + i] + x[i]) - cs[i]; }
    k[0] += 1.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) { k[1 + i] += s[i]; k[4 + i] += d[i]; }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) k[7 + r * 3 + c] += s[r] * d[c];
}

// Kabsch from shifted sums k[16] = {cnt, sum(s-cs)[3], sum(d-cd)[3], sum (s-cs)(d-cd)^T [9]}.
__device__ __noinline__ int kabsch_finish(const double* k, const double cs[3], const double cd[3], int reflection,
                          double* out) {
    const double n = k[0];
    if (!(n > 0.0)) return SSF_POSE_EMPTY;
    double es[3], ed[3], ms[3], md[3];
    for (int i = 0; i < 3; ++i) {
        es[i] = k[1 + i] / n; ed[i] = k[4 + i] / n;
        ms[i] = cs[i] + es[i]; md[i] = cd[i] + ed[i];
    }
    double H[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) H[r * 3 + c] = k[7 + r * 3 + c] - n * es[r] * ed[c];
    double U[9], Sv[3], Vt[9], R[9];
    svd3(H, U, Sv, Vt);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double s = 0.0;
            for (int j = 0; j < 3; ++j) s += Vt[j * 3 + r] * U[c * 3 + j];
            R[r * 3 + c] = s;
        }
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) +
                       R[2] * (R[3] * R[7] - R[4] * R[6]);
    int status = 0;
    if (det < 0) {
        if (!reflection) status = SSF_POSE_REFLECTION;
        for (int j = 0; j < 3; ++j) Vt[6 + j] *= -1.0;
        if (reflection)
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) {
                    double s = 0.0;
                    for (int j = 0; j < 3; ++j) s += Vt[j * 3 + r] * U[c * 3 + j];
                    R[r * 3 + c] = s;
                }
    }
    double t[3];
    for (int r = 0; r < 3; ++r) t[r] = -(R[r * 3] * ms[0] + R[r * 3 + 1] * ms[1] + R[r * 3 + 2] * ms[2]) + md[r];
    // pyquaternion Quaternion(matrix=R): orthogonality check, trace method on m = R^T
    bool orth = true;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int kk = 0; kk < 3; ++kk) s += R[i * 3 + kk] * R[j * 3 + kk];
            const double e = (i == j) ? 1.0 : 0.0;
            if (!(fabs(s - e) <= 1e-8 + 1e-5 * fabs(e))) orth = false;
        }
    double q[4] = {0, 0, 0, 0};
    if (orth) {
        double m[3][3];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) m[i][j] = R[j * 3 + i];
        double tt, w, x, y, z;
        if (m[2][2] < 0) {
            if (m[0][0] > m[1][1]) {
                tt = 1 + m[0][0] - m[1][1] - m[2][2];
                w = m[1][2] - m[2][1]; x = tt; y = m[0][1] + m[1][0]; z = m[2][0] + m[0][2];
            } else {
                tt = 1 - m[0][0] + m[1][1] - m[2][2];
                w = m[2][0] - m[0][2]; x = m[0][1] + m[1][0]; y = tt; z = m[1][2] + m[2][1];
            }
        } else {
            if (m[0][0] < -m[1][1]) {
                tt = 1 - m[0][0] - m[1][1] + m[2][2];
                w = m[0][1] - m[1][0]; x = m[2][0] + m[0][2]; y = m[1][2] + m[2][1]; z = tt;
            } else {
                tt = 1 + m[0][0] + m[1][1] + m[2][2];
                w = tt; x = m[1][2] - m[2][1]; y = m[2][0] - m[0][2]; z = m[0][1] - m[1][0];
            }
        }
        const double f = 0.5 / sqrt(tt);
        q[0] = x * f; q[1] = y * f; q[2] = z * f; q[3] = w * f;
    } else if (status == 0) {
        status = SSF_POSE_NOT_ORTHOGONAL;
    }
    for (int i = 0; i < 3; ++i) out[SSF_POSE_OUT_T + i] = t[i];
    for (int i = 0; i < 4; ++i) out[SSF_POSE_OUT_Q + i] = q[i];
    for (int i = 0; i < 9; ++i) out[SSF_POSE_OUT_R + i] = R[i];
    out[SSF_POSE_OUT_NBG] = n;
    return status;
}

}  // namespace ssf
