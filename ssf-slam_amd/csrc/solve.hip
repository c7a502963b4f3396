// solve.hip -- the solve of frameRegistration (src/lidarOdometry_onlyPC.cpp:147-252) on gfx950,
// batched over independent frame pairs, and launch_register, which chains a registration's
// stages: the association (associate.hip), the edge association (edges.hip), the solve.
//
//   k_solve               one work-group per pair runs the whole Ceres-LM or GN loop on device
//                         (one instantiation per mode): residual / Jacobian / Huber evaluation
//                         in f64 over the records in LDS, deterministic block reduction of the
//                         28 normal-equation terms, and the 6x6 step redundantly in every
//                         thread -- no host round trip and no lane-0 section between iterations.
//   k_accumulate          chains relative poses into absolute ones.
#include "ssf_device.hpp"
#include "ssf_internal.hpp"

#include <float.h>

namespace ssf {

// one wave per SIMD: the per-pair solve is latency-bound (a block reduction and a 6x6 solve per
// iteration), and 256 threads measured 0.083 ms per 256-pair launch against 0.092 at 512 and
// 0.28 at 1024 (round 2c, tools/gpu/r2c_solve3.sh).  For a launch of ONE pair (BASELINE
// configs[1] as written) 512 threads were slower too: 0.083 against 0.073 ms (round 3,
// tools/gpu/r3g.sh; 1024 threads cap the solve at 128 VGPRs and spill).
#ifndef SSF_SOLVE_THREADS
#define SSF_SOLVE_THREADS 256
#endif
constexpr int kSolveThreads = SSF_SOLVE_THREADS;
constexpr int kNE = 28;  // 21 (packed upper JtWJ) + 6 (JtWr) + cost

SSF_DEV int pk(int u, int v) {
    if (u > v) { int t = u; u = v; v = t; }
    return u * 6 - (u * (u - 1)) / 2 + (v - u);
}

// All threads: evaluate Huber(0.1)-corrected normal equations at (q, t) over the pair's
// records; result (x2 for the reference's duplicated residual blocks) in ne[] of every thread.
// Valid correspondences of a pair compacted (original order) into LDS once per solve, SoA floats:
// every evaluation of the LM/GN loop then reads LDS instead of re-streaming the 48-byte records.
constexpr int kSolveLdsCap = 4096;
#ifndef SSF_SOLVE_CMP_PER
#define SSF_SOLVE_CMP_PER 8
#endif
constexpr int kCmpPer = SSF_SOLVE_CMP_PER;        // records per thread and pass of it
struct CorrLds {
    float po[3][kSolveLdsCap], pa[3][kSolveLdsCap], n[3][kSolveLdsCap];
};

// Eigen Quaterniond::toRotationMatrix (x, y, z, w storage).
SSF_DEV void quat_to_R(const double q[4], double R[9]) {
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
    R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}

// 1 / sqrt(s) (s > 0, normal): v_rsq_f64 and two Newton steps, r <- r + r (1 - s r^2) / 2; the
// pivot is d = s r (sqrt(s)) and its reciprocal r -- one short chain instead of the f64 sqrt and
// divide expansions on the solve's critical path (every thread runs it)
SSF_DEV double rsq_refined(double s) {
    double r = __builtin_amdgcn_rsq(s);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double e = __builtin_fma(-s * r, r, 1.0);
        r = __builtin_fma(0.5 * r, e, r);
    }
    return r;
}

// The rotational Jacobian columns carry a factor 2 (the quaternion parameterisation below).
// It is applied to the block sums instead of every correspondence: every
// product and partial sum of those entries is then exactly 2 or 4 times the unscaled one (a
// power-of-two scaling commutes with rounding), so the sums are bit-identical and each
// correspondence saves three f64 multiplies.  kNeScale folds it into the evaluation's final x2
// (the duplicated residual blocks): packed J^T W J entries (u, v) x4 (u, v < 3) / x2 (u < 3 <= v)
// / x1, J^T W r entries x2 (u < 3), the cost x1 -- each times that 2.
__device__ constexpr double kNeScale[kNE] = {8, 8, 8, 4, 4, 4, 8, 8, 4, 4, 4, 8, 4, 4, 4, 2, 2, 2, 2, 2, 2,
                                             4, 4, 4, 2, 2, 2, 2};
// Per-correspondence residual r = (R po + t - pa) . n (PlaneFeatureCost, :25-43) and its local
// Jacobian [2 (R po x n), n]: the EigenQuaternionParameterization's 4x3 Jacobian composed with
// the autodiff gradient (what the oracle's residual_jac spells out) reduces to that for a unit
// quaternion, so an evaluation costs ~65 f64 operations per correspondence instead of ~140 (same
// values to rounding, explicit FMAs; the per-step poses keep the 1e-5 m / 1e-6 rad bar against
// the oracle).  R is built once per evaluation (wave-uniform).  Huber(0.1) corrector as Ceres:
// rho'(s) = 0.1 / sqrt(s) above s = 0.01 (sqrt(r^2) taken as |r|), rho(s) = 0.2 sqrt(s) - 0.01.
// One correspondence's Huber-weighted contribution (x wgt: 0 for a padding slot) to the
// normal equations ne (21 packed upper J^T W J, 6 J^T W r, cost).
SSF_DEV void accum_corr(const double R[9], const double t[3], const double po[3], const double pa[3],
                        const double nn[3], double wgt, double (&ne)[kNE]) {
    const double a = 0.1, b = 0.1 * 0.1;
    double u[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] = __builtin_fma(R[3 * k + 2], po[2], __builtin_fma(R[3 * k + 1], po[1], R[3 * k] * po[0]));
    const double d0 = (u[0] + t[0]) - pa[0], d1 = (u[1] + t[1]) - pa[1], d2 = (u[2] + t[2]) - pa[2];
    const double r = __builtin_fma(d2, nn[2], __builtin_fma(d1, nn[1], d0 * nn[0]));
    double J[6];
    J[0] = __builtin_fma(u[1], nn[2], -u[2] * nn[1]);
    J[1] = __builtin_fma(u[2], nn[0], -u[0] * nn[2]);
    J[2] = __builtin_fma(u[0], nn[1], -u[1] * nn[0]);
    J[3] = nn[0]; J[4] = nn[1]; J[5] = nn[2];
    const double s = r * r;
    double rho0, rho1;
    if (s > b) {
        const double rr = fabs(r);
        rho0 = 2.0 * a * rr - b;
        rho1 = a / rr;
        if (rho1 < DBL_MIN) rho1 = DBL_MIN;
    } else {
        rho0 = s; rho1 = 1.0;
    }
    ne[27] = __builtin_fma(0.5 * wgt, rho0, ne[27]);
    rho1 *= wgt;
    int k = 0;
#pragma unroll
    for (int uu = 0; uu < 6; ++uu) {             // explicit FMAs: the file is built without
        const double wj = rho1 * J[uu];          // contraction (bit-exact float stages)
        ne[21 + uu] = __builtin_fma(wj, r, ne[21 + uu]);
#pragma unroll
        for (int v = uu; v < 6; ++v) { ne[k] = __builtin_fma(wj, J[v], ne[k]); ++k; }
    }
}

// Point-to-line block (beyond the reference): e = P (R po + t - c), P = I - u u^T; row k is the
// plane residual with "normal" P row k, so its local Jacobian is [2 (R po x P_k), P_k]; one
// Huber(0.1) block on s = |e|^2 (rho'(s) = 0.1 / sqrt(s) above s = 0.01).
SSF_DEV void accum_edge(const double R[9], const double t[3], const double po[3], const double c[3],
                        const double uu[3], double wgt, double (&ne)[kNE]) {
    const double a = 0.1, b = 0.1 * 0.1;
    double g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = __builtin_fma(R[3 * k + 2], po[2], __builtin_fma(R[3 * k + 1], po[1], R[3 * k] * po[0]));
    const double d[3] = {(g[0] + t[0]) - c[0], (g[1] + t[1]) - c[1], (g[2] + t[2]) - c[2]};
    double r[3], J[3][6], s = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double nk[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) nk[j] = (j == k ? 1.0 : 0.0) - uu[k] * uu[j];
        r[k] = __builtin_fma(d[2], nk[2], __builtin_fma(d[1], nk[1], d[0] * nk[0]));
        J[k][0] = __builtin_fma(g[1], nk[2], -g[2] * nk[1]);
        J[k][1] = __builtin_fma(g[2], nk[0], -g[0] * nk[2]);
        J[k][2] = __builtin_fma(g[0], nk[1], -g[1] * nk[0]);
        J[k][3] = nk[0]; J[k][4] = nk[1]; J[k][5] = nk[2];
        s = __builtin_fma(r[k], r[k], s);
    }
    double rho0, rho1;
    if (s > b) {
        const double rr = sqrt(s);
        rho0 = 2.0 * a * rr - b;
        rho1 = a / rr;
        if (rho1 < DBL_MIN) rho1 = DBL_MIN;
    } else {
        rho0 = s; rho1 = 1.0;
    }
    ne[27] = __builtin_fma(0.5 * wgt, rho0, ne[27]);
    rho1 *= wgt;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int m = 0;
#pragma unroll
        for (int uu2 = 0; uu2 < 6; ++uu2) {
            const double wj = rho1 * J[k][uu2];
            ne[21 + uu2] = __builtin_fma(wj, r[k], ne[21 + uu2]);
#pragma unroll
            for (int v = uu2; v < 6; ++v) { ne[m] = __builtin_fma(wj, J[k][v], ne[m]); ++m; }
        }
    }
}

SSF_DEV void evaluate(const CorrRec* __restrict__ rec, int n, const double q[4], const double t[3],
                      double (&ne)[kNE], double* lds, const CorrRec* __restrict__ erec = nullptr,
                      int en = 0) {
#pragma unroll
    for (int k = 0; k < kNE; ++k) ne[k] = 0.0;
    double R[9];
    quat_to_R(q, R);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const CorrRec c = rec[i];
        if (c.valid == 0.0f) continue;
        const double po[3] = {c.po[0], c.po[1], c.po[2]}, pa[3] = {c.pa[0], c.pa[1], c.pa[2]},
                     nn[3] = {c.n[0], c.n[1], c.n[2]};
        accum_corr(R, t, po, pa, nn, 1.0, ne);
    }
    for (int i = threadIdx.x; i < en; i += blockDim.x) {          // edge blocks (en = 0: none)
        const CorrRec c = erec[i];
        if (c.valid == 0.0f) continue;
        const double po[3] = {c.po[0], c.po[1], c.po[2]}, pa[3] = {c.pa[0], c.pa[1], c.pa[2]},
                     uu[3] = {c.n[0], c.n[1], c.n[2]};
        accum_edge(R, t, po, pa, uu, 1.0, ne);
    }
    block_sum_rs<kNE>(ne, lds);
#pragma unroll
    for (int k = 0; k < kNE; ++k) ne[k] *= kNeScale[k];
}

// LDS-resident correspondences, kSolveStep per step (i, i + T, ...; a missing one is a clamped
// duplicate weighted 0): all of a step's loads are in flight before the first is used.
#ifndef SSF_SOLVE_STEP
#define SSF_SOLVE_STEP 2
#endif
constexpr int kSolveStep = SSF_SOLVE_STEP;
template <int NW>
SSF_DEV void evaluate(const CorrLds& C, int nv, const double q[4], const double t[3],
                      double (&ne)[kNE], double* lds, int nve = 0, int parity = 0) {
#pragma unroll
    for (int k = 0; k < kNE; ++k) ne[k] = 0.0;
    double R[9];
    quat_to_R(q, R);
    const int T = blockDim.x;
    for (int i = threadIdx.x; i < nv; i += kSolveStep * T) {
        float f[kSolveStep][9];
#pragma unroll
        for (int h = 0; h < kSolveStep; ++h) {
            const int ih = min(i + h * T, nv - 1);
#pragma unroll
            for (int d = 0; d < 3; ++d) { f[h][d] = C.po[d][ih]; f[h][3 + d] = C.pa[d][ih]; f[h][6 + d] = C.n[d][ih]; }
        }
#pragma unroll
        for (int h = 0; h < kSolveStep; ++h) {
            const double po[3] = {f[h][0], f[h][1], f[h][2]}, pa[3] = {f[h][3], f[h][4], f[h][5]},
                         nn[3] = {f[h][6], f[h][7], f[h][8]};
            accum_corr(R, t, po, pa, nn, (h == 0 || i + h * T < nv) ? 1.0 : 0.0, ne);
        }
    }
    for (int i = nv + threadIdx.x; i < nv + nve; i += T) {        // edge blocks after the planes
        const double po[3] = {C.po[0][i], C.po[1][i], C.po[2][i]}, pa[3] = {C.pa[0][i], C.pa[1][i], C.pa[2][i]},
                     uu[3] = {C.n[0][i], C.n[1][i], C.n[2][i]};
        accum_edge(R, t, po, pa, uu, 1.0, ne);
    }
    block_sum_db<kNE, NW>(ne, lds, parity);
#pragma unroll
    for (int k = 0; k < kNE; ++k) ne[k] *= kNeScale[k];
}

// The first evaluation over records the association compacted ([0, nv) of rec, rank order, all
// valid, 1 <= nv <= kSolveLdsCap -- the clamped loads need a record): evaluate<NW>()'s loop -- the same records per thread in the same
// order and the same sums -- with each record read from global memory and stored to the LDS
// arrays the later evaluations read (positions i + h T of thread t are read back by thread t
// only: no barrier).  The loads of a step are in flight together; the first evaluation's
// arithmetic overlaps the stream that the ballot compaction used to wait for alone.
template <int NW>
SSF_DEV void evaluate_load(const CorrRec* __restrict__ rec, CorrLds& C, int nv, const double q[4],
                           const double t[3], double (&ne)[kNE], double* lds, int parity) {
#pragma unroll
    for (int k = 0; k < kNE; ++k) ne[k] = 0.0;
    double R[9];
    quat_to_R(q, R);
    const int T = blockDim.x;
    // one step's records in flight ahead of the step being evaluated (clamped, unconditional
    // loads: a step past nv re-reads record nv - 1 and is never used)
    float4 n0[kSolveStep], n1[kSolveStep], n2[kSolveStep];
#pragma unroll
    for (int h = 0; h < kSolveStep; ++h) {
        const float4* rp = reinterpret_cast<const float4*>(rec + min((int)threadIdx.x + h * T, nv - 1));
        n0[h] = rp[0]; n1[h] = rp[1]; n2[h] = rp[2];
    }
    for (int i = threadIdx.x; i < nv; i += kSolveStep * T) {
        float4 r0[kSolveStep], r1[kSolveStep], r2[kSolveStep];
#pragma unroll
        for (int h = 0; h < kSolveStep; ++h) {
            r0[h] = n0[h]; r1[h] = n1[h]; r2[h] = n2[h];
            const float4* rp = reinterpret_cast<const float4*>(rec + min(i + kSolveStep * T + h * T, nv - 1));
            n0[h] = rp[0]; n1[h] = rp[1]; n2[h] = rp[2];
        }
#pragma unroll
        for (int h = 0; h < kSolveStep; ++h) {
            const int ih = i + h * T;
            if (ih < nv) {
                C.po[0][ih] = r0[h].x; C.po[1][ih] = r0[h].y; C.po[2][ih] = r0[h].z;
                C.pa[0][ih] = r1[h].x; C.pa[1][ih] = r1[h].y; C.pa[2][ih] = r1[h].z;
                C.n[0][ih] = r2[h].x; C.n[1][ih] = r2[h].y; C.n[2][ih] = r2[h].z;
            }
            const double po[3] = {r0[h].x, r0[h].y, r0[h].z}, pa[3] = {r1[h].x, r1[h].y, r1[h].z},
                         nn[3] = {r2[h].x, r2[h].y, r2[h].z};
            accum_corr(R, t, po, pa, nn, (h == 0 || ih < nv) ? 1.0 : 0.0, ne);
        }
    }
    block_sum_db<kNE, NW>(ne, lds, parity);
#pragma unroll
    for (int k = 0; k < kNE; ++k) ne[k] *= kNeScale[k];
}

// quat_plus for a GN step: |d| = theta < 2^-7 (a step of a converging solve) takes sin(theta) /
// theta and cos(theta) as their Taylor polynomials in theta^2 = |d|^2 -- no sqrt, division, sin or
// cos on the per-iteration critical path every thread runs.  The first omitted terms are below
// 2^-95 (sinc, x2^5 / 11!) and 2^-112 (cos, x2^6 / 12!) of the results, far under one f64 ulp
// (2^-53): the values agree with libm's to an ulp or so, as libm agrees with the oracle's glibc.
// Larger steps take quat_plus itself.
SSF_DEV void quat_plus_step(const double q[4], const double d[3], double o[4]) {
    const double x2 = __builtin_fma(d[2], d[2], __builtin_fma(d[1], d[1], d[0] * d[0]));
    if (x2 > 0.0 && x2 < 0x1p-14) {
        // Horner in x2: sinc = sum (-x2)^k / (2k + 1)!, k <= 4; cos = sum (-x2)^k / (2k)!, k <= 5
        double sc = 1.0 / 362880.0;
        sc = __builtin_fma(sc, x2, -1.0 / 5040.0);
        sc = __builtin_fma(sc, x2, 1.0 / 120.0);
        sc = __builtin_fma(sc, x2, -1.0 / 6.0);
        sc = __builtin_fma(sc, x2, 1.0);
        double c = -1.0 / 3628800.0;
        c = __builtin_fma(c, x2, 1.0 / 40320.0);
        c = __builtin_fma(c, x2, -1.0 / 720.0);
        c = __builtin_fma(c, x2, 1.0 / 24.0);
        c = __builtin_fma(c, x2, -0.5);
        c = __builtin_fma(c, x2, 1.0);
        const double dq[4] = {sc * d[0], sc * d[1], sc * d[2], c};
        quat_mul(dq, q, o);
        return;
    }
    quat_plus(q, d, o);
}

// Cholesky solve of the packed symmetric normal equations A y = -g (A = ne[0..20] upper packed,
// g = ne[21..26]): 21 + 21 doubles of state, one reciprocal per diagonal instead of a division
// per element (the GN path runs it redundantly on every thread).
// a - b c, as one fused operation (a shorter dependent chain; the step moves by rounding only)
SSF_DEV double msub(double a, double b, double c) {
    return __builtin_fma(-b, c, a);
}
SSF_DEV int chol_solve_packed(const double (&ne)[kNE], double y[6]) {
    double L[21];                         // L(i, j), j <= i, at pk(j, i)
    double inv[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = ne[pk(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) s = msub(s, L[pk(k, j)], L[pk(k, j)]);
        if (!(s > 0.0)) return -1;
        const double r = (s > 1e-290 && s < 1e290) ? rsq_refined(s) : 1.0 / sqrt(s);
        const double d = (s > 1e-290 && s < 1e290) ? s * r : sqrt(s);
        inv[j] = r;
        L[pk(j, j)] = d;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = ne[pk(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) v = msub(v, L[pk(k, i)], L[pk(k, j)]);
            L[pk(j, i)] = v * inv[j];
        }
    }
    double z[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = -ne[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = msub(v, L[pk(k, i)], z[k]);
        z[i] = v * inv[i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = z[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v = msub(v, L[pk(i, k)], y[k]);
        y[i] = v * inv[i];
    }
    return 0;
}

struct SolveShared {       // the pair's pose and log length, from the solve to thread 0's output
    double q[4], t[3];
    int nlog;
};

SSF_DEV void write_log(double* log, int max_iter, int p, int idx, const double q[4],
                       const double t[3], double cost, double status, double radius) {
    if (!log || idx >= max_iter) return;
    double* r = log + ((int64_t)p * max_iter + idx) * 10;
    r[0] = q[0]; r[1] = q[1]; r[2] = q[2]; r[3] = q[3];
    r[4] = t[0]; r[5] = t[1]; r[6] = t[2];
    r[7] = cost; r[8] = status; r[9] = radius;
}

// kEdges: point-to-line blocks (ecorr at ecurr_off / ecurr_count) join every evaluation; they
// are compacted into the same LDS arrays after the planes.
// kMode: the solver this instantiation runs (SSF_SOLVER_GN / SSF_SOLVER_CERES_LM), so each mode's
// register allocation covers its own loop only (the LM state does not weigh on the GN kernel).
// The launch still passes the mode as an argument; the kernel does not read it.
template <bool kEdges, int NT, int kMode>
__global__ __launch_bounds__(NT) void k_solve(const CorrRec* __restrict__ corr,
                                                         const int64_t* __restrict__ curr_off,
                                                         const int32_t* __restrict__ curr_count,
                                                         const int32_t* __restrict__ last_count,
                                                         int /*mode*/, int max_iter,
                                                         const double* pose_in,
                                                         const double* pose_abs_in,
                                                         double* pose_rel,
                                                         double* pose_abs,
                                                         double* __restrict__ log,
                                                         int32_t* __restrict__ nlog_out,
                                                         int32_t* __restrict__ ncorr_out,
                                                         const CorrRec* __restrict__ ecorr,
                                                         const int64_t* __restrict__ ecurr_off,
                                                         const int32_t* __restrict__ ecurr_count,
                                                         int32_t* __restrict__ ncorr_edge_out,
                                                         const int32_t* __restrict__ ncompact) {
    __shared__ SolveShared S;
    __shared__ double red[2 * (NT / 64 + 1) * kNE];                   // block_sum_db: two halves
    __shared__ CorrLds C;
    __shared__ int wtot2[2][NT / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = curr_count[p];
    const CorrRec* rec = corr + curr_off[p];
    // records the association already compacted (ncompact[p] >= 0): read with the other per-pair
    // scalars, before the first barrier
    const int ncp = (!kEdges && ncompact) ? ncompact[p] : -1;          // uniform
    const int en = kEdges ? ecurr_count[p] : 0;
    const CorrRec* erec = kEdges ? ecorr + ecurr_off[p] : nullptr;
#ifdef SSF_SOLVE_STAMPS
    // diagnostic build only: s_memtime phase stamps into the last log row (cost/status/radius)
    const unsigned long long st0 = __builtin_amdgcn_s_memtime();
    unsigned long long st1 = st0, st2 = st0;
#endif
#ifdef SSF_SOLVE_STAMPS2
    // diagnostic build only: the GN iterations split into the 6x6 solve + pose update and the
    // evaluation (replacing the compaction / first-evaluation stamps of the log row)
    unsigned long long t_sol = 0, t_ev = 0;
#endif
    if (tid == 0) {
        for (int k = 0; k < 4; ++k) S.q[k] = pose_in[7 * p + k];
        for (int k = 0; k < 3; ++k) S.t[k] = pose_in[7 * p + 4 + k];
        S.nlog = 0;
    }
    __syncthreads();
    const bool skip = last_count[p] <= 10;                              // :158
    if (!skip) {
        // order-preserving compaction of the valid records into LDS, coalesced:
        const int lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
        const int T = blockDim.x;
        // one pass per kCmpPer x T records: wave w takes a contiguous range of kCmpPer x 64, every
        // load of the pass in flight at once; per 64-record step a ballot, the ranks from the
        // wave's own popcounts and ONE exchange of the wave totals (one barrier per pass; the
        // totals alternate between two LDS rows, so the next pass needs no second barrier)
        auto compact = [&](const CorrRec* __restrict__ src, int cnt, int start) {
            int nv = 0;                                                 // uniform
            for (int i0 = 0, ps = 0; i0 < cnt; i0 += kCmpPer * T, ps ^= 1) {
                const int wb = i0 + w * kCmpPer * 64;
                float4 c0[kCmpPer], c1[kCmpPer], c2[kCmpPer];
#pragma unroll
                for (int j = 0; j < kCmpPer; ++j) {
                    const CorrRec* r = src + min(wb + j * 64 + lane, cnt - 1);   // clamped
                    c0[j] = reinterpret_cast<const float4*>(r)[0];
                    c1[j] = reinterpret_cast<const float4*>(r)[1];
                    c2[j] = reinterpret_cast<const float4*>(r)[2];
                }
                uint64_t m[kCmpPer];
                int wt = 0;
#pragma unroll
                for (int j = 0; j < kCmpPer; ++j) {
                    m[j] = __ballot(wb + j * 64 + lane < cnt && c0[j].w != 0.0f);
                    wt += __popcll(m[j]);
                }
                if (lane == 0) wtot2[ps][w] = wt;
                __syncthreads();
                int before = start + nv, tot = 0;
                for (int j = 0; j < nw; ++j) { const int x = wtot2[ps][j]; if (j < w) before += x; tot += x; }
#pragma unroll
                for (int j = 0; j < kCmpPer; ++j) {
                    const int pos = before + __popcll(m[j] & lanemask_lt());
                    if (((m[j] >> lane) & 1ull) && pos < kSolveLdsCap) {
                        C.po[0][pos] = c0[j].x; C.po[1][pos] = c0[j].y; C.po[2][pos] = c0[j].z;
                        C.pa[0][pos] = c1[j].x; C.pa[1][pos] = c1[j].y; C.pa[2][pos] = c1[j].z;
                        C.n[0][pos] = c2[j].x; C.n[1][pos] = c2[j].y; C.n[2][pos] = c2[j].z;
                    }
                    before += __popcll(m[j]);
                }
                nv += tot;
            }
            __syncthreads();                                            // the LDS records, for every wave
            return nv;
        };
        // compacted records: [0, ncp) in rank order, streamed into LDS by the first evaluation
        // itself (evaluate_load: the same per-thread order and sums as evaluate() from LDS), no
        // ballot pass
        const int nv = ncp >= 0 ? ncp : compact(rec, n, 0);
        const int nve = kEdges ? compact(erec, en, nv) : 0;
        const bool in_lds = nv + nve <= kSolveLdsCap;                  // uniform
#ifdef SSF_SOLVE_STAMPS
        st1 = __builtin_amdgcn_s_memtime();
#endif
        if (tid == 0 && ncorr_out) ncorr_out[p] = nv;
        if (kEdges && tid == 0 && ncorr_edge_out) ncorr_edge_out[p] = nve;
        int par = 0;                                                    // block_sum_dpp's LDS half
        // (compacted records beyond the LDS: every record of [0, nv) is valid)
        const int nglob = ncp >= 0 ? nv : n;
        auto eval_at = [&](const double* qq, const double* tt, double (&ne_)[kNE]) {
            if (in_lds) evaluate<NT / 64>(C, nv, qq, tt, ne_, red, nve, par);
            else evaluate(rec, nglob, qq, tt, ne_, red, erec, en);
            par ^= 1;
        };
        double ne[kNE];
        double q[4], t[3];
        for (int k = 0; k < 4; ++k) q[k] = S.q[k];
        for (int k = 0; k < 3; ++k) t[k] = S.t[k];
        // (nv == 0 -- an empty current frame, or no valid correspondence -- has no record to load:
        // evaluate_load's clamped loads would read rec[-1]; evaluate() from LDS gives the zero sums)
        if (ncp > 0 && in_lds) {
            evaluate_load<NT / 64>(rec, C, nv, q, t, ne, red, par);
            par ^= 1;
        } else {
            eval_at(q, t, ne);
        }
#ifdef SSF_SOLVE_STAMPS
        st2 = __builtin_amdgcn_s_memtime();
#endif
        if (kMode == SSF_SOLVER_GN) {
            // every thread holds the same sums after the block reduction, so every thread runs
            // the same 6x6 solve on the same bits and carries the same pose: no lane-0 step, no
            // LDS broadcast, no extra barrier per iteration (thread 0 alone writes the log)
            int nl = 0;
            for (int it = 0; it < max_iter; ++it) {
                double y[6];
#ifdef SSF_SOLVE_STAMPS2
                const unsigned long long sa = __builtin_amdgcn_s_memtime();
#endif
                if (chol_solve_packed(ne, y) != 0) {                         // uniform
                    if (tid == 0) write_log(log, max_iter, p, nl, q, t, ne[27], 2, 0);
                    ++nl;
                    break;
                }
                double qn[4];
                quat_plus_step(q, y, qn);
                for (int k = 0; k < 4; ++k) q[k] = qn[k];
                t[0] += y[3]; t[1] += y[4]; t[2] += y[5];
#ifdef SSF_SOLVE_STAMPS2
                const unsigned long long sb = __builtin_amdgcn_s_memtime();
#endif
                eval_at(q, t, ne);
#ifdef SSF_SOLVE_STAMPS2
                const unsigned long long sc = __builtin_amdgcn_s_memtime();
                t_sol += sb - sa; t_ev += sc - sb;
#endif
                if (tid == 0) write_log(log, max_iter, p, nl, q, t, ne[27], 6, 0);
                ++nl;
            }

            if (tid == 0) {
                for (int k = 0; k < 4; ++k) S.q[k] = q[k];
                for (int k = 0; k < 3; ++k) S.t[k] = t[k];
                S.nlog = nl;
            }
            __syncthreads();
        } else {
            // every thread carries the LM state (accepted pose and normal equations, scaling,
            // radius) in registers and runs the same step on the same bits, as the GN path does:
            // no lane-0 section that the other 255 threads wait on at two barriers per iteration,
            // no LDS round trips on the serial chain, the 6x6 solve by rsq pivots
            double qa[4], ta[3], na[kNE], sc[6];
            for (int k = 0; k < 4; ++k) qa[k] = q[k];
            for (int k = 0; k < 3; ++k) ta[k] = t[k];
#pragma unroll
            for (int k = 0; k < kNE; ++k) na[k] = ne[k];
#pragma unroll
            for (int u = 0; u < 6; ++u) sc[u] = 1.0 / (1.0 + sqrt(ne[pk(u, u)]));
            double radius = 1e4, dec = 2.0;
            int invalid = 0, nl = 0;
            for (int it = 1; it <= max_iter; ++it) {
                // LevenbergMarquardtStrategy::ComputeStep on the Jacobi-scaled system: m holds
                // M = As + diag(clamp(As_uu)) / radius packed, and gs, so chol_solve_packed
                // solves M y = -gs
                double As[21], m[kNE], y[6];
#pragma unroll
                for (int u = 0; u < 6; ++u) {
                    m[21 + u] = sc[u] * na[21 + u];
#pragma unroll
                    for (int v = u; v < 6; ++v) As[pk(u, v)] = sc[u] * na[pk(u, v)] * sc[v];
                }
#pragma unroll
                for (int k = 0; k < 21; ++k) m[k] = As[k];
#pragma unroll
                for (int u = 0; u < 6; ++u) {
                    double d = As[pk(u, u)];
                    if (d < 1e-6) d = 1e-6;
                    if (d > 1e32) d = 1e32;
                    m[pk(u, u)] += d / radius;
                }
                const bool ok = chol_solve_packed(m, y) == 0;             // uniform
                double mcc = 0.0;
                if (ok) {
                    double yg = 0.0, yAy = 0.0;
#pragma unroll
                    for (int u = 0; u < 6; ++u) {
                        yg += y[u] * m[21 + u];
                        double Ay = 0.0;
#pragma unroll
                        for (int v = 0; v < 6; ++v) Ay += As[pk(u, v)] * y[v];
                        yAy += y[u] * Ay;
                    }
                    mcc = -(yg + 0.5 * yAy);
                }
                if (!ok || !(mcc > 0.0)) {
                    radius /= dec; dec *= 2.0;
                    if (tid == 0) write_log(log, max_iter, p, nl, qa, ta, na[27], 2, radius);
                    ++nl;
                    if (++invalid > 5) break;
                    continue;
                }
                invalid = 0;
                double delta[6], qc[4], tc[3];
#pragma unroll
                for (int u = 0; u < 6; ++u) delta[u] = y[u] * sc[u];
                quat_plus_step(qa, delta, qc);
                tc[0] = ta[0] + delta[3]; tc[1] = ta[1] + delta[4]; tc[2] = ta[2] + delta[5];
                eval_at(qc, tc, ne);
                double xn = 0.0, sn = 0.0;
                for (int u = 0; u < 4; ++u) { xn += qa[u] * qa[u]; sn += (qa[u] - qc[u]) * (qa[u] - qc[u]); }
                for (int u = 0; u < 3; ++u) { xn += ta[u] * ta[u]; sn += (ta[u] - tc[u]) * (ta[u] - tc[u]); }
                xn = sqrt(xn); sn = sqrt(sn);
                const double dcost = na[27] - ne[27];
                if (!(sn > (xn + 1e-8) * 1e-8)) {                       // ParameterToleranceReached
                    if (tid == 0) write_log(log, max_iter, p, nl, qa, ta, na[27], 3, radius);
                    ++nl;
                    break;
                }
                if (!(fabs(dcost) > 1e-6 * na[27])) {                   // FunctionToleranceReached
                    if (tid == 0) write_log(log, max_iter, p, nl, qa, ta, na[27], 4, radius);
                    ++nl;
                    break;
                }
                const double rho = dcost / mcc;
                if (rho > 1e-3) {                                       // accept
                    for (int k = 0; k < 4; ++k) qa[k] = qc[k];
                    for (int k = 0; k < 3; ++k) ta[k] = tc[k];
#pragma unroll
                    for (int k = 0; k < kNE; ++k) na[k] = ne[k];
                    const double f = 2.0 * rho - 1.0;
                    double den = 1.0 - f * f * f;
                    if (den < 1.0 / 3.0) den = 1.0 / 3.0;
                    radius = radius / den;
                    if (radius > 1e16) radius = 1e16;
                    dec = 2.0;
                    const double mg[3] = {-ne[21], -ne[22], -ne[23]};
                    double qg[4], gm = 0.0;
                    quat_plus(qa, mg, qg);
                    for (int u = 0; u < 4; ++u) gm = fmax(gm, fabs(qa[u] - qg[u]));
                    for (int u = 3; u < 6; ++u) gm = fmax(gm, fabs(ne[21 + u]));
                    const bool conv = gm <= 1e-10;                      // GradientToleranceReached
                    if (tid == 0) write_log(log, max_iter, p, nl, qa, ta, na[27], conv ? 5 : 1, radius);
                    ++nl;
                    if (conv) break;
                } else {                                                // reject
                    radius /= dec; dec *= 2.0;
                    if (tid == 0) write_log(log, max_iter, p, nl, qa, ta, na[27], 0, radius);
                    ++nl;
                }
            }
            if (tid == 0) {
                for (int k = 0; k < 4; ++k) S.q[k] = qa[k];
                for (int k = 0; k < 3; ++k) S.t[k] = ta[k];
                S.nlog = nl;
            }
        }
    } else if (tid == 0) {
        if (ncorr_out) ncorr_out[p] = -1;
        if (kEdges && ncorr_edge_out) ncorr_edge_out[p] = -1;
    }
    if (tid == 0) {
#ifdef SSF_SOLVE_STAMPS
        if (log) {
            double* r = log + ((int64_t)p * max_iter + max_iter - 1) * 10;
#ifdef SSF_SOLVE_STAMPS2
            r[7] = (double)t_sol; r[8] = (double)t_ev;
#else
            r[7] = (double)(st1 - st0); r[8] = (double)(st2 - st1);
#endif
            r[9] = (double)(__builtin_amdgcn_s_memtime() - st2);
        }
#endif
        for (int k = 0; k < 4; ++k) pose_rel[7 * p + k] = S.q[k];
        for (int k = 0; k < 3; ++k) pose_rel[7 * p + 4 + k] = S.t[k];
        if (nlog_out) nlog_out[p] = S.nlog;
        if (pose_abs) {                                                 // :87-90
            double q0l[4], t0l[3], q0c[4], r[3];
            for (int k = 0; k < 4; ++k) q0l[k] = pose_abs_in[7 * p + k];
            for (int k = 0; k < 3; ++k) t0l[k] = pose_abs_in[7 * p + 4 + k];
            quat_mul(q0l, S.q, q0c);
            quat_rotate(q0l, S.t, r);
            for (int k = 0; k < 4; ++k) pose_abs[7 * p + k] = q0c[k];
            for (int k = 0; k < 3; ++k) pose_abs[7 * p + 4 + k] = t0l[k] + r[k];
        }
    }
}

__global__ void k_accumulate(int n, const double* __restrict__ rel, const double* __restrict__ start,
                             double* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
    if (start) {
        for (int k = 0; k < 4; ++k) q[k] = start[k];
        for (int k = 0; k < 3; ++k) t[k] = start[4 + k];
    }
    for (int i = 0; i < n; ++i) {
        const double* r = rel + 7 * i;
        double qn[4], rt[3];
        quat_mul(q, r, qn);
        quat_rotate(q, r + 4, rt);
        for (int k = 0; k < 3; ++k) t[k] = t[k] + rt[k];
        for (int k = 0; k < 4; ++k) q[k] = qn[k];
        for (int k = 0; k < 4; ++k) out[7 * i + k] = q[k];
        for (int k = 0; k < 3; ++k) out[7 * i + 4 + k] = t[k];
    }
}

// The solve launch of launch_register: warm starts / start poses read from pin / ain, results
// written to a.pose.rel / a.pose.abs; ncp: the compacted-record counts the association wrote,
// else nullptr.
void launch_solve(hipStream_t s, const ssf_config& cfg, int n_pairs, const RegisterArgs& a,
                  const double* pin, const double* ain, int32_t* ncp) {
    const EdgeReg* edge = a.edge;
    kmark(s, "k_solve");
#define SSF_SOLVE_LAUNCH(E, NT, ...)                                                               \
    hipLaunchKernelGGL((cfg.solver == SSF_SOLVER_GN ? k_solve<E, NT, SSF_SOLVER_GN> : k_solve<E, NT, SSF_SOLVER_CERES_LM>), \
                       dim3(n_pairs), dim3(NT), 0, s, a.scratch.corr, a.curr.off, a.curr.count, \
                       a.last.count, cfg.solver, cfg.max_iter, pin, ain, a.pose.rel, a.pose.abs, a.out.log, \
                       a.out.nlog, a.out.ncorr, __VA_ARGS__, ncp)
    if (edge)
        SSF_SOLVE_LAUNCH(true, kSolveThreads, edge->corr, edge->curr_off, edge->curr_count, edge->ncorr);
    else
        SSF_SOLVE_LAUNCH(false, kSolveThreads, (const CorrRec*)nullptr, (const int64_t*)nullptr,
                         (const int32_t*)nullptr, (int32_t*)nullptr);
#undef SSF_SOLVE_LAUNCH
}

hipError_t launch_register(hipStream_t s, const ssf_config& cfg, int n_pairs, const RegisterArgs& a) {
    if (n_pairs <= 0) return hipSuccess;
    // warm starts / start poses read from pose.in / pose.abs_in (null: in place), results
    // written to pose.rel / pose.abs: a chain reads pair k - 1's output slot directly
    const double* pin = a.pose.in ? a.pose.in : a.pose.rel;
    const double* ain = a.pose.abs_in ? a.pose.abs_in : a.pose.abs;
    // compacted records (k_associate_strips' lane mode with one work-group per pair, planes only):
    // the association writes the counts, the solve reads them; otherwise neither sees them
    int32_t* ncp = nullptr;
    if (a.max_m > 0) {
        RegisterPlan plan = register_plan(n_pairs, a.max_m, a.edge != nullptr);
        plan.strips = plan.strips && a.table.sorted && a.table.sidx;
        plan.compacted = plan.strips && plan.compacted && a.scratch.nnv && a.scratch.ncompact;
        if (plan.compacted) ncp = a.scratch.ncompact;
        launch_associate(s, n_pairs, plan, a, pin);
    }
    if (a.edge && a.edge->max_m > 0) launch_edge_associate(s, n_pairs, a.edge, pin);
    launch_solve(s, cfg, n_pairs, a, pin, ain, ncp);
    return hipGetLastError();
}

hipError_t launch_accumulate(hipStream_t s, int n, const double* rel, const double* start,
                             double* abs_out) {
    if (n <= 0) return hipSuccess;
    kmark(s, "k_accumulate");
    hipLaunchKernelGGL(k_accumulate, dim3(1), dim3(64), 0, s, n, rel, start, abs_out);
    return hipGetLastError();
}

}  // namespace ssf
