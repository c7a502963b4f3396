// reg_knn.hpp -- device helpers shared by the registration stages (plane_table.hip,
// associate.hip, edges.hip): the 5x3 least-squares plane of a 30-NN list, the packed (distance,
// index) keys with their sorted insertion, the ring row of a point and transformToLast.
#pragma once
#include "ssf_device.hpp"

#include <float.h>

namespace ssf {

// Eigen ColPivHouseholderQR<Matrix<float,5,3>>::solve(-1) -- same sequence as the oracle's
// qr_solve_5x3 (oracle/ssf_oracle.c), float, no FMA contraction.
SSF_DEV float sqnorm_f(const float* v, int n) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < n; ++i) s = s + v[i] * v[i];
    return s;
}

// Every loop is unrolled and every runtime index (the pivot column, the permutation, the rank)
// is applied as a predicate on compile-time indices: the 5x3 system stays in registers (with
// runtime indices it lived in scratch, ~90 B of private-memory traffic per plane point).  The
// floating-point operations and their order are those of the oracle's loops.
SSF_DEV void qr_solve_5x3(float m[3][5], float x[3]) {
    float hc[3] = {0.f, 0.f, 0.f};
    int tr[3] = {0, 1, 2};
    float nu[3], nd[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { nd[k] = sqrtf(sqnorm_f(m[k], 5)); nu[k] = nd[k]; }
    float mx = nu[0];
#pragma unroll
    for (int k = 1; k < 3; ++k) if (nu[k] > mx) mx = nu[k];
    float th = mx * FLT_EPSILON;
    th = (th * th) / 5.0f;
    const float ndt = sqrtf(FLT_EPSILON);
    int nz = 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int bi = k;
        float bv = nu[k];
#pragma unroll
        for (int j = k + 1; j < 3; ++j) if (nu[j] > bv) { bv = nu[j]; bi = j; }
        const float bsq = bv * bv;
        if (nz == 3 && bsq < th * (float)(5 - k)) nz = k;
        tr[k] = bi;
#pragma unroll
        for (int j = k + 1; j < 3; ++j) {
            if (j == bi) {
#pragma unroll
                for (int r = 0; r < 5; ++r) { float t = m[k][r]; m[k][r] = m[j][r]; m[j][r] = t; }
                float t = nu[k]; nu[k] = nu[j]; nu[j] = t;
                t = nd[k]; nd[k] = nd[j]; nd[j] = t;
            }
        }
        constexpr int L0 = 5;
        const int L = L0 - k;
        float* v = &m[k][k];
        const float tail = sqnorm_f(v + 1, L - 1);
        const float c0 = v[0];
        float beta, tau;
        if (tail <= FLT_MIN) {
            tau = 0.0f; beta = c0;
#pragma unroll
            for (int i = 1; i < L; ++i) v[i] = 0.0f;
        } else {
            beta = sqrtf(c0 * c0 + tail);
            if (c0 >= 0.0f) beta = -beta;
            const float den = c0 - beta;
#pragma unroll
            for (int i = 1; i < L; ++i) v[i] = v[i] / den;
            tau = (beta - c0) / beta;
        }
        hc[k] = tau;
        v[0] = beta;
        if (tau != 0.0f) {
#pragma unroll
            for (int c = k + 1; c < 3; ++c) {
                float tmp = 0.0f;
#pragma unroll
                for (int i = 1; i < L; ++i) tmp = tmp + v[i] * m[c][k + i];
                tmp = tmp + m[c][k];
                m[c][k] = m[c][k] - tau * tmp;
#pragma unroll
                for (int i = 1; i < L; ++i) m[c][k + i] = m[c][k + i] - (tau * v[i]) * tmp;
            }
        }
#pragma unroll
        for (int j = k + 1; j < 3; ++j) {
            if (nu[j] != 0.0f) {
                float t = fabsf(m[j][k]) / nu[j];
                t = (1.0f + t) * (1.0f - t);
                if (t < 0.0f) t = 0.0f;
                const float rr = nu[j] / nd[j];
                const float t2 = t * (rr * rr);
                if (t2 <= ndt) {
                    nd[j] = sqrtf(sqnorm_f(&m[j][k + 1], 5 - k - 1));
                    nu[j] = nd[j];
                } else {
                    nu[j] = nu[j] * sqrtf(t);
                }
            }
        }
    }
    int perm[3] = {0, 1, 2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {                       // swap perm[k] and perm[tr[k]] (tr[k] >= k)
        const int pk0 = perm[k];
        int pt = pk0;
#pragma unroll
        for (int j = k; j < 3; ++j) if (j == tr[k]) pt = perm[j];
#pragma unroll
        for (int j = k; j < 3; ++j) if (j == tr[k]) perm[j] = pk0;
        perm[k] = pt;
    }
    x[0] = x[1] = x[2] = 0.0f;
    if (nz == 0) return;
    float c[5] = {-1.0f, -1.0f, -1.0f, -1.0f, -1.0f};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k >= nz) break;
        const float tau = hc[k];
        const int L = 5 - k;
        if (tau != 0.0f) {
            const float* v = &m[k][k];
            float tmp = 0.0f;
#pragma unroll
            for (int i = 1; i < L; ++i) tmp = tmp + v[i] * c[k + i];
            tmp = tmp + c[k];
            c[k] = c[k] - tau * tmp;
#pragma unroll
            for (int i = 1; i < L; ++i) c[k + i] = c[k + i] - (tau * v[i]) * tmp;
        }
    }
#pragma unroll
    for (int i = 2; i >= 0; --i) {
        if (i < nz && c[i] != 0.0f) {
            c[i] = c[i] / m[i][i];
#pragma unroll
            for (int s2 = 0; s2 < i; ++s2) c[s2] = c[s2] - c[i] * m[i][s2];
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int p2 = 0; p2 < 3; ++p2)
            if (i < nz && perm[i] == p2) x[p2] = c[i];
}

constexpr int kKnnTile = 2048;
constexpr int kK = 30;

SSF_DEV bool lex_less(float ka, int ia, float kb, int ib) { return ka < kb || (ka == kb && ia < ib); }

SSF_DEV float l2_simple(const float4& q, const float4& p) {
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    float d = dx * dx + dy * dy;
    return d + dz * dz;
}

// A (distance, index) pair packed into one f64: high word = the non-negative f32 distance
// bits, low word = the index.  For non-negative, non-NaN values the f64 order is the u64 order
// of the bits, i.e. exactly the lexicographic (distance, index) order, so a sorted insertion is
// one v_min_f64 + one v_max_f64 per slot.  (Keys with distance 0 are f64 denormals; the kernel
// keeps f64 denormals, the default, so they compare correctly.)
SSF_DEV double knn_key(float d, int id) { return __hiloint2double(__float_as_int(d), id); }
SSF_DEV float key_dist(double k) { return __int_as_float(__double2hiint(k)); }
SSF_DEV int key_index(double k) { return __double2loint(k); }

// Branch-free.  Measured and reverted (round 2d): skipping the slots when no active lane's key
// beats its list's last (exact: keys are unique) made k_plane_table_sorted 0.40 -> 0.67 ms.
template <int K>
SSF_DEV void key_insert(double (&kk)[K], double key) {
#pragma unroll
    for (int s = 0; s < K; ++s) {
        // plain v_max/v_min (keys are never NaN: no canonicalisation), the slot updated in place
        double hi;
        asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(kk[s]), "v"(key));
        asm("v_min_f64 %0, %0, %1" : "+v"(kk[s]) : "v"(key));
        key = hi;
    }
}
// key_insert that returns the key leaving the list (the new key itself when it does not enter)
template <int K>
SSF_DEV double key_insert_out(double (&kk)[K], double key) {
#pragma unroll
    for (int s = 0; s < K; ++s) {
        double hi;
        asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(kk[s]), "v"(key));
        asm("v_min_f64 %0, %0, %1" : "+v"(kk[s]) : "v"(key));
        key = hi;
    }
    return key;
}

// Ring-diverse 5-point pick (:180-205), gate d2[n] < 1 (:207), 5x3 least-squares plane
// (:208-220) and coplanarity gate (:222-232) from the sorted 30-NN key list kk of a point.
SSF_DEV void plane_from_knn(const float4* __restrict__ P, const double (&kk)[30],
                            int m, float plane_max, float nrm[3], uint8_t& ok) {
    const int K = m < 30 ? m : 30;
    nrm[0] = nrm[1] = nrm[2] = 0.f;
    ok = 0;
    if (K < 5) return;                                                 // :177
    int v5[5];
    int prow = -1, vr0 = -1, vr1 = -1, nvr = 0, n = 5;
#pragma unroll
    for (int ik = 0; ik < 30; ++ik) {                                  // :180-198
        if (ik < K && nvr < 2) {
            const int id = key_index(kk[ik]);
            if ((unsigned)id >= (unsigned)m) { ok = 0; return; }       // never reached: lists are complete
            const float fi = P[id].w;
            const int ii = (int)fi;
            const int row = (int)(100.0 * ((double)(fi - (float)ii) + 0.002));
            if (ik == 0) prow = row;
            if (ik < 5) {
                v5[ik] = id;
            } else if (row != prow && row >= 0 && row <= 63) {
                if (nvr == 0) vr0 = id; else vr1 = id;
                nvr++;
                n = ik;
            }
        }
    }
    if (nvr == 1) v5[4] = vr0;                                         // :199-205
    if (nvr == 2) { v5[3] = vr0; v5[4] = vr1; }
    float dn = key_dist(kk[0]);
#pragma unroll
    for (int ik = 0; ik < 30; ++ik) if (ik == n) dn = key_dist(kk[ik]);
    if (!(dn < 1.0f)) return;                                          // :207
    float Am[3][5];
    float pts[5][3];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const float4 p = P[v5[j]];
        pts[j][0] = p.x; pts[j][1] = p.y; pts[j][2] = p.z;
        Am[0][j] = p.x; Am[1][j] = p.y; Am[2][j] = p.z;
    }
    qr_solve_5x3(Am, nrm);                                             // :219
    float z = nrm[0] * nrm[0] + nrm[1] * nrm[1];
    z = z + nrm[2] * nrm[2];
    if (z > 0.0f) {                                                    // :220
        const float sq = sqrtf(z);
        nrm[0] = nrm[0] / sq; nrm[1] = nrm[1] / sq; nrm[2] = nrm[2] / sq;
    }
    ok = 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                      // :222-232
        const double vx = (double)(pts[k][0] - pts[k + 1][0]);
        const double vy = (double)(pts[k][1] - pts[k + 1][1]);
        const double vz = (double)(pts[k][2] - pts[k + 1][2]);
        double dd = (double)nrm[0] * vx + (double)nrm[1] * vy;
        dd = dd + (double)nrm[2] * vz;
        if (fabs(dd) > (double)plane_max) { ok = 0; break; }
    }
}

SSF_DEV int row_of(float fi) {                           // lidarOdometry_onlyPC.cpp:181-183
    const int ii = (int)fi;
    return (int)(100.0 * ((double)(fi - (float)ii) + 0.002));
}

// The current point in the last frame's coordinates (transformToLast, f64 rotation).
SSF_DEV float4 assoc_query_point(const float4& pc, const double q[4], const double t[3]) {
    const double v[3] = {(double)pc.x, (double)pc.y, (double)pc.z};
    double r[3];
    quat_rotate(q, v, r);                                               // :74-82
    float4 qs;
    qs.x = (float)(r[0] + t[0]); qs.y = (float)(r[1] + t[1]); qs.z = (float)(r[2] + t[2]); qs.w = 0.f;
    return qs;
}

}  // namespace ssf
