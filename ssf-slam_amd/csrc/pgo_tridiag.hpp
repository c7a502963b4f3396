// pgo_tridiag.hpp -- the block-tridiagonal part T of the pose-graph Hessian (prior + edges with
// |i - j| == 1): assemble it with the gradient, factor it (block Cholesky), and solve with it
// (pgo_substitute, one right-hand side per lane).
#pragma once
#include "pgo_common.hpp"

namespace ssf {

// Assemble T as diagonal blocks D_k and sub-diagonal blocks O_k = H[k+1][k], and the gradient GR
// over every factor: one thread per node, edges in order (a fixed summation order); the edge
// index pairs are staged through LDS in tiles, so the scan reads no global memory.  A chain link
// without an edge sets bit 0 of S.fail.  kLM: T is damped by D / radius.  Ends with a barrier.
template <bool kLM>
SSF_DEV void pgo_assemble(const PgoCtx& c, PgoLdsCommon& S, double radius) {
    const int tid = c.tid, K = c.K, E = c.E;
    const double* REC = c.REC;
    for (int kb = 0; kb < K; kb += kPgoThreads) {                      // uniform
        const int k = kb + tid;
        const bool act = k < K;
        double Dk[36], Ok[36], gk[6];
        for (int q = 0; q < 36; ++q) { Dk[q] = 0.0; Ok[q] = 0.0; }
        for (int q = 0; q < 6; ++q) gk[q] = 0.0;
        double hd[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // step control: the loop rows' part of diag(J^T J)
        bool linked = false;
        auto add = [&](int e, int i, int j) {      // factor e touches node k (e < 0: the prior)
            const double* rec = REC + (size_t)kPgoRec * (e < 0 ? E : e);
            const double* Jk = rec + (i == k ? 6 : 42);
            const bool chain = e < 0 || i - j == 1 || j - i == 1;
            const int other = i == k ? j : i;
            const bool next = e >= 0 && chain && other == k + 1;
            const double* Jo = rec + (i == k ? 42 : 6);
            linked = linked || next;
            // one Jacobian row at a time: rank-1 updates of g, D (lower) and O
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                double jk[6];
#pragma unroll
                for (int a = 0; a < 6; ++a) jk[a] = Jk[6 * q + a];
                const double rc = rec[q];
#pragma unroll
                for (int a = 0; a < 6; ++a) gk[a] += jk[a] * rc;
                if (chain) {
#pragma unroll
                    for (int a = 0; a < 6; ++a)
#pragma unroll
                        for (int b = 0; b <= a; ++b) Dk[6 * a + b] += jk[a] * jk[b];
                }
                if constexpr (kLM) {
                    if (!chain) {
#pragma unroll
                        for (int a = 0; a < 6; ++a) hd[a] += jk[a] * jk[a];
                    }
                }
                if (next) {
#pragma unroll
                    for (int a = 0; a < 6; ++a) {
                        const double jo = Jo[6 * q + a];
#pragma unroll
                        for (int b = 0; b < 6; ++b) Ok[6 * a + b] += jo * jk[b];
                    }
                }
            }
        };
        if (k == 0) add(-1, -2, 0);                // the prior: the dj form on node 0
        for (int e0 = 0; e0 < E; e0 += kPgoTile) {                     // uniform
            const int tn = min(kPgoTile, E - e0);
            __syncthreads();
            for (int t = tid; t < tn; t += kPgoThreads)
                S.ij[t] = make_int2(c.IJ[2 * (e0 + t)], c.IJ[2 * (e0 + t) + 1]);
            __syncthreads();
            if (act)
                for (int t = 0; t < tn; ++t) {
                    const int2 ij = S.ij[t];
                    if (ij.x == k || ij.y == k) add(e0 + t, ij.x, ij.y);
                }
        }
        if constexpr (kLM) {
            // H + D / radius, D = the diagonal of the full J^T J (chain edges, prior and the scaled
            // loop rows) clamped to [1e-6, 1e32]: it lands on T, the Woodbury form stays
#pragma unroll
            for (int a = 0; a < 6; ++a) Dk[7 * a] += fmin(fmax(Dk[7 * a] + hd[a], 1e-6), 1e32) / radius;
        }
        if (act) {
            for (int q = 0; q < 36; ++q) { c.D[36 * (size_t)k + q] = Dk[q]; c.O[36 * (size_t)k + q] = Ok[q]; }
            for (int q = 0; q < 6; ++q) c.GR[6 * (size_t)k + q] = gk[q];
            // a chain link without an edge: T is singular (in exact arithmetic; rounding
            // could let its Cholesky pass), whatever the loop edges connect
            if (k + 1 < K && !linked) atomicOr(&S.fail, 1);
        }
    }
    __syncthreads();
}

// Block Cholesky of T on one lane: D_k <- L_k (lower, reciprocal diagonal), O_k <- M_k =
// O_k L_k^-T.  A failed pivot sets S.fail (kLM: bit 1; bit 0 stays the missing chain link's).
// Ends with a barrier.
template <bool kLM>
SSF_DEV void pgo_block_cholesky(const PgoCtx& c, PgoLdsCommon& S) {
    const int K = c.K;
    double* D = c.D;
    double* O = c.O;
    if (c.tid == 0) {
        double M[36], Dn[36];                      // Dn: the next node's diagonal block, loaded ahead
        int ok = 1;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b) Dn[6 * a + b] = D[6 * a + b];
        for (int k = 0; k < K && ok; ++k) {
            double Sm[36], Oc[36];                 // Oc is used last: its load hides behind the factor
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = 0; b < 6; ++b) {
                    if (b <= a) Sm[6 * a + b] = Dn[6 * a + b];
                    Oc[6 * a + b] = O[36 * (size_t)k + 6 * a + b];
                }
            if (k + 1 < K) {
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = 0; b <= a; ++b) Dn[6 * a + b] = D[36 * (size_t)(k + 1) + 6 * a + b];
            }
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b) {
                    double s = Sm[6 * a + b];
                    if (k > 0)
#pragma unroll
                        for (int q = 0; q < 6; ++q) s -= M[6 * a + q] * M[6 * b + q];
                    Sm[6 * a + b] = s;
                }
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                double p = Sm[6 * b + b];
#pragma unroll
                for (int q = 0; q < b; ++q) p -= Sm[6 * b + q] * Sm[6 * b + q];
                if (!(p > 0.0) || !pgo_finite(p)) { ok = 0; break; }
                const double inv = 1.0 / sqrt(p);
#pragma unroll
                for (int a = b + 1; a < 6; ++a) {
                    double s = Sm[6 * a + b];
#pragma unroll
                    for (int q = 0; q < b; ++q) s -= Sm[6 * a + q] * Sm[6 * b + q];
                    Sm[6 * a + b] = s * inv;
                }
                Sm[6 * b + b] = inv;
            }
            if (!ok) break;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b) D[36 * (size_t)k + 6 * a + b] = Sm[6 * a + b];
            if (k + 1 < K) {
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = 0; b < 6; ++b) {
                        double s = Oc[6 * a + b];
#pragma unroll
                        for (int q = 0; q < b; ++q) s -= M[6 * a + q] * Sm[6 * b + q];
                        M[6 * a + b] = s * Sm[6 * b + b];
                    }
#pragma unroll
                for (int q = 0; q < 36; ++q) O[36 * (size_t)k + q] = M[q];
            }
        }
        if constexpr (kLM) {
            if (!ok) S.fail |= 2;
        } else {
            if (!ok) S.fail = 1;
        }
    }
    __syncthreads();
}

// T^-1 of one column on one lane: forward and back substitution through the block factors
// (D: L_k with reciprocal diagonal, O: M_k), serial over the nodes.  The column lives at
// z[(6 k + r) * zs]; the block factors are read one step ahead of their use.
SSF_DEV void pgo_substitute(const double* D, const double* O, int K, double* z, size_t zs, const PgoColumn& rhs) {
    double y[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    // Ln / Mn: the blocks of the next step (L_k and the M that couples it to the step
    // before), loaded while the current step computes
    double Ln[36], Mn[36];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            if (c <= a) Ln[6 * a + c] = D[6 * a + c];
            Mn[6 * a + c] = 0.0;
        }
    for (int k = 0; k < K; ++k) {
        double Lk[36], M[36];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                if (c <= a) Lk[6 * a + c] = Ln[6 * a + c];
                M[6 * a + c] = Mn[6 * a + c];
            }
        if (k + 1 < K) {
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    if (c <= a) Ln[6 * a + c] = D[36 * (size_t)(k + 1) + 6 * a + c];
                    Mn[6 * a + c] = O[36 * (size_t)(k) + 6 * a + c];
                }
        }
        double b[6];
        rhs(k, b);
        if (k > 0) {
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) b[r] -= M[6 * r + c] * y[c];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double s = b[r];
#pragma unroll
            for (int c = 0; c < r; ++c) s -= Lk[6 * r + c] * y[c];
            y[r] = s * Lk[6 * r + r];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) z[(6 * (size_t)k + r) * zs] = y[r];
    }
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double bn[6];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            if (c <= a) Ln[6 * a + c] = D[36 * (size_t)(K - 1) + 6 * a + c];
            Mn[6 * a + c] = 0.0;
        }
#pragma unroll
    for (int r = 0; r < 6; ++r) bn[r] = z[(6 * (size_t)(K - 1) + r) * zs];
    for (int k = K - 1; k >= 0; --k) {
        double Lk[36], M[36];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                if (c <= a) Lk[6 * a + c] = Ln[6 * a + c];
                M[6 * a + c] = Mn[6 * a + c];
            }
        double b[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) b[r] = bn[r];
        if (k > 0) {
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    if (c <= a) Ln[6 * a + c] = D[36 * (size_t)(k - 1) + 6 * a + c];
                    Mn[6 * a + c] = O[36 * (size_t)(k - 1) + 6 * a + c];
                }
#pragma unroll
            for (int r = 0; r < 6; ++r) bn[r] = z[(6 * (size_t)(k - 1) + r) * zs];
        }
        if (k + 1 < K) {
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) b[r] -= M[6 * c + r] * x[c];
        }
#pragma unroll
        for (int r = 5; r >= 0; --r) {
            double s = b[r];
#pragma unroll
            for (int c = r + 1; c < 6; ++c) s -= Lk[6 * c + r] * x[c];
            x[r] = s * Lk[6 * r + r];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) z[(6 * (size_t)k + r) * zs] = x[r];
    }
}

}  // namespace ssf
