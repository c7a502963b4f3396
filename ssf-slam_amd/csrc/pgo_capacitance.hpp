// pgo_capacitance.hpp -- the loop edges of the pose-graph solver by Woodbury: the substitutions
// T^-1 [ -g | A^T ], the capacitance matrix C = I + A T^-1 A^T (order n = 6 L, column-major in
// CM), its dense Cholesky and the step dx = T^-1 b - T^-1 A^T C^-1 A T^-1 b, left in column 0 of
// Z.  One function per path; each returns true when a pivot of C failed (uniform over the
// work-group; there is no step then) and gives every thread the max-norm of its part of dx in
// mx (infinite for a non-finite entry).
#pragma once
#include "pgo_tridiag.hpp"

namespace ssf {

// Up to kPgoNarrowLoops loops: every right-hand side on a lane of its own, the loop list and the
// capacitance vectors in LDS, the Cholesky with one thread per row.
SSF_DEV bool pgo_capacitance_narrow(const PgoCtx& c, PgoLds<false>& S, double& mx) {
    const int tid = c.tid, K = c.K, L = c.L, n = c.n, NC = c.NC;
    const double* REC = c.REC;
    double* Z = c.Z;
    double* CM = c.CM;
    // -- T^-1 [ -g | A^T ]: one lane per column, serial over the nodes
    if (tid < NC) {
        const int col = tid, l = col > 0 ? (col - 1) / 6 : 0, row = col > 0 ? (col - 1) % 6 : 0;
        const int li = col > 0 ? S.loop_i[l] : -1, lj = col > 0 ? S.loop_j[l] : -1;
        const double* lrec = REC + (size_t)kPgoRec * (col > 0 ? S.loop_e[l] : 0);
        pgo_substitute(c.D, c.O, K, Z + col, c.zs, PgoColumn{col, row, li, lj, lrec, c.GR});
    }
    __syncthreads();

    // -- Woodbury: C = I + A Z_A, u = A z0, C w = u
    if (L > 0) {
        if (tid < n) {
            const int l = tid / 6, row = tid % 6;
            const double* lrec = REC + (size_t)kPgoRec * S.loop_e[l];
            const double* zi = Z + 6 * (size_t)S.loop_i[l] * NC;
            const double* zj = Z + 6 * (size_t)S.loop_j[l] * NC;
            for (int b = 0; b <= n; ++b) {                 // b == 0: u; b >= 1: column b - 1
                double s = 0.0;
                for (int q = 0; q < 6; ++q)
                    s += lrec[6 + 6 * row + q] * zi[(size_t)q * NC + b] + lrec[42 + 6 * row + q] * zj[(size_t)q * NC + b];
                if (b == 0) S.va[tid] = s;
                else CM[(size_t)(b - 1) * n + tid] = s + (b - 1 == tid ? 1.0 : 0.0);
            }
        }
        __syncthreads();
        bool failed = false;
        for (int j = 0; j < n; ++j) {                      // Cholesky, one thread per row
            double s = 0.0;
            if (tid < n && tid >= j) {
                s = CM[(size_t)j * n + tid];
                for (int p = 0; p < j; ++p) s -= CM[(size_t)p * n + tid] * CM[(size_t)p * n + j];
                if (tid == j) S.piv = s;
            }
            __syncthreads();
            const double piv = S.piv;
            if (!(piv > 0.0) || !pgo_finite(piv)) { failed = true; break; }   // uniform
            if (tid < n && tid >= j) CM[(size_t)j * n + tid] = tid == j ? sqrt(piv) : s / sqrt(piv);
            __syncthreads();
        }
        if (failed) return true;
        for (int j = 0; j < n; ++j) {                      // forward: va -> vb
            __syncthreads();
            const double yj = S.va[j] / CM[(size_t)j * n + j];
            if (tid == j) S.vb[j] = yj;
            if (tid < n && tid > j) S.va[tid] -= CM[(size_t)j * n + tid] * yj;
        }
        for (int j = n - 1; j >= 0; --j) {                 // backward: vb -> va
            __syncthreads();
            const double xj = S.vb[j] / CM[(size_t)j * n + j];
            if (tid == j) S.va[j] = xj;
            if (tid < j) S.vb[tid] -= CM[(size_t)tid * n + j] * xj;
        }
        __syncthreads();
    }

    // -- dx = z0 - Z_A w (into column 0) and its max-norm
    for (int k = tid; k < K; k += kPgoThreads)
        for (int r = 0; r < 6; ++r) {
            double* zr = Z + (6 * (size_t)k + r) * NC;
            double s = zr[0];
            for (int b = 0; b < n; ++b) s -= zr[1 + b] * S.va[b];
            zr[0] = s;
            mx = pgo_finite(s) ? fmax(mx, fabs(s)) : __builtin_inf();
        }
    return false;
}

// Up to SSF_PGO_MAX_LOOPS loops: the loop list (LP), C and its vectors (VA: u, then w; VB) in
// the graph's scratch, everything sized by L.
SSF_DEV bool pgo_capacitance_wide(const PgoCtx& c, PgoLds<true>& S, double& mx) {
    const int tid = c.tid, K = c.K, L = c.L, n = c.n, NC = c.NC;
    const size_t zs = c.zs;
    const int32_t* LP = c.LP;
    const double* REC = c.REC;
    double* Z = c.Z;
    double* CM = c.CM;
    double* VA = c.VA;
    double* VB = c.VB;
    // -- T^-1 [ -g | A^T ], kPgoThreads columns a pass, one lane per column.  A lane folds its
    //    solved column into the capacitance matrix (column 0, z0 = T^-1 (-g), into u = A z0)
    //    before the pass buffer is reused: T^-1 A^T is never held whole.  A lane reads back only
    //    what it wrote itself: no barrier in here.
    for (int c0 = 0; c0 < NC; c0 += kPgoThreads) {
        const int col = c0 + tid;
        if (col < NC) {
            const int l = col > 0 ? (col - 1) / 6 : 0, row = col > 0 ? (col - 1) % 6 : 0;
            const int li = col > 0 ? LP[3 * l + 1] : -1, lj = col > 0 ? LP[3 * l + 2] : -1;
            const double* lrec = REC + (size_t)kPgoRec * (col > 0 ? LP[3 * l] : 0);
            double* z = Z + tid;
            pgo_substitute(c.D, c.O, K, z, zs, PgoColumn{col, row, li, lj, lrec, c.GR});
            for (int m = 0; m < L; ++m) {                  // rows 6 m .. 6 m + 5 of A z
                const double* mrec = REC + (size_t)kPgoRec * LP[3 * m];
                const double* zi = z + 6 * (size_t)LP[3 * m + 1] * zs;
                const double* zj = z + 6 * (size_t)LP[3 * m + 2] * zs;
                double vi[6], vj[6];
                for (int q = 0; q < 6; ++q) { vi[q] = zi[(size_t)q * zs]; vj[q] = zj[(size_t)q * zs]; }
                for (int r = 0; r < 6; ++r) {
                    double s = 0.0;
                    for (int q = 0; q < 6; ++q) s += mrec[6 + 6 * r + q] * vi[q] + mrec[42 + 6 * r + q] * vj[q];
                    if (col == 0) VA[6 * m + r] = s;
                    else CM[(size_t)(col - 1) * n + 6 * m + r] = s + (col - 1 == 6 * m + r ? 1.0 : 0.0);
                }
            }
        }
    }
    __syncthreads();

    // -- Woodbury: C w = u by dense Cholesky, the rows strided over the threads (row
    //    tid + q kPgoThreads in slot q), then dx = T^-1 (-g - A^T w).  Left-looking by
    //    panels of kPgoPanel columns: a sweep over the columns left of the panel updates the
    //    whole panel, so C is read n / kPgoPanel times, not n times.  A slot takes part while
    //    any of its rows does (a uniform test); its rows above the diagonal read a clamped
    //    address and their sums are never stored.
    if (L > 0) {
        bool failed = false;
        for (int j0 = 0; j0 < n; j0 += kPgoPanel) {
            // t: the thread index made opaque, so that the row offsets below are not hoisted out
            // of the iteration loop into registers the substitution phases need
            int t = tid;
            asm volatile("" : "+v"(t));
            double acc[kPgoWideRows][kPgoPanel];
#pragma unroll
            for (int q = 0; q < kPgoWideRows; ++q)
#pragma unroll
                for (int b = 0; b < kPgoPanel; ++b) {
                    const int r = t + q * kPgoThreads;
                    acc[q][b] = r < n && r >= j0 && j0 + b < n ? CM[(size_t)(j0 + b) * n + r] : 0.0;
                }
            for (int p = 0; p < j0; ++p) {
                double cj[kPgoPanel];
#pragma unroll
                for (int b = 0; b < kPgoPanel; ++b) cj[b] = CM[(size_t)p * n + min(j0 + b, n - 1)];
#pragma unroll
                for (int q = 0; q < kPgoWideRows; ++q)
                    if (q * kPgoThreads < n && (q + 1) * kPgoThreads > j0) {
                        const double cr = CM[(size_t)p * n + min(t + q * kPgoThreads, n - 1)];
#pragma unroll
                        for (int b = 0; b < kPgoPanel; ++b) acc[q][b] -= cr * cj[b];
                    }
            }
#pragma unroll
            for (int b = 0; b < kPgoPanel; ++b) {          // the panel's own columns in turn
                const int j = j0 + b;
                if (j >= n) break;
#pragma unroll
                for (int a = 0; a < b; ++a) {
                    const double cja = CM[(size_t)(j0 + a) * n + j];
#pragma unroll
                    for (int q = 0; q < kPgoWideRows; ++q) acc[q][b] -= acc[q][a] * cja;
                }
#pragma unroll
                for (int q = 0; q < kPgoWideRows; ++q)
                    if (t + q * kPgoThreads == j) S.piv = acc[q][b];
                __syncthreads();
                const double piv = S.piv;
                if (!(piv > 0.0) || !pgo_finite(piv)) { failed = true; break; }   // uniform
#pragma unroll
                for (int q = 0; q < kPgoWideRows; ++q) {
                    const int r = t + q * kPgoThreads;
                    acc[q][b] = r == j ? sqrt(piv) : acc[q][b] / sqrt(piv);
                    if (r < n && r >= j) CM[(size_t)j * n + r] = acc[q][b];
                }
                __syncthreads();
            }
            if (failed) break;
        }
        if (failed) return true;
        for (int j = 0; j < n; ++j) {                      // forward: VA -> VB
            __syncthreads();
            const double yj = VA[j] / CM[(size_t)j * n + j];
            if (tid == j % kPgoThreads) VB[j] = yj;
            for (int r = tid; r < n; r += kPgoThreads)
                if (r > j) VA[r] -= CM[(size_t)j * n + r] * yj;
        }
        for (int j = n - 1; j >= 0; --j) {                 // backward: VB -> VA
            __syncthreads();
            const double xj = VB[j] / CM[(size_t)j * n + j];
            if (tid == j % kPgoThreads) VA[j] = xj;
            for (int r = tid; r < j; r += kPgoThreads) VB[r] -= CM[(size_t)r * n + j] * xj;
        }
        __syncthreads();
        // g + A^T w at the loop nodes in loop order, then one more column: -(g + A^T w)
        if (tid == 0) {
            for (int m = 0; m < L; ++m) {
                const double* mrec = REC + (size_t)kPgoRec * LP[3 * m];
                double* gi = c.GR + 6 * (size_t)LP[3 * m + 1];
                double* gj = c.GR + 6 * (size_t)LP[3 * m + 2];
                for (int q = 0; q < 6; ++q) {
                    double si = 0.0, sj = 0.0;
                    for (int r = 0; r < 6; ++r) {
                        si += mrec[6 + 6 * r + q] * VA[6 * m + r];
                        sj += mrec[42 + 6 * r + q] * VA[6 * m + r];
                    }
                    gi[q] += si;
                    gj[q] += sj;
                }
            }
            pgo_substitute(c.D, c.O, K, Z, zs, PgoColumn{0, 0, -1, -1, REC, c.GR});
        }
        __syncthreads();
    }
    for (int k = tid; k < K; k += kPgoThreads)
        for (int r = 0; r < 6; ++r) {
            const double s = Z[(6 * (size_t)k + r) * zs];
            mx = pgo_finite(s) ? fmax(mx, fabs(s)) : __builtin_inf();
        }
    return false;
}

}  // namespace ssf
