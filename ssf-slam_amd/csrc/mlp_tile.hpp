// The f32-MFMA tile of the grouped MLPs, shared by k_grouped_mlp_max
// (pointnet2.hip) and k_grouped_mlp (cost_volume.hip), and the error plumbing of the
// ssf_pn2_* entry points (one thread-local message, read by ssf_pn2_last_error).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ssf_device.hpp"

namespace ssf_pn2_detail {
// defined in pointnet2.hip: record the calling thread's message and return the code
int32_t fail(int32_t code, const char* msg);
int32_t hip_status(hipError_t e, const char* what);
}  // namespace ssf_pn2_detail

namespace {

constexpr int kMlpThreads = 512;
constexpr int kMlpWaves = kMlpThreads / 64;
constexpr int kMlpStage = 32 * 33;             // floats per wave of last-layer staging
constexpr int kMlpLdsMax = 160 * 1024;
constexpr int kMlpUnroll = 8;                  // MFMA k-steps whose operands are loaded together

typedef float f16v __attribute__((ext_vector_type(16)));

extern __shared__ float mlp_lds[];

// acc = W[:, o0 .. o0 + 32)^T X[:, c0 .. c0 + 32) over the w_in input channels, k ascending; X is
// the [channel][tc] image at float offset x0 of the work-group's LDS
SSF_DEV f16v mlp_tile(const float* __restrict__ W, int w_in, int w_out, int o0, int x0, int tc,
                      int c0, int lane) {
    const int r = lane & 31, h = lane >> 5;
    const int o = o0 + r;
    const bool ov = o < w_out;
    const unsigned wc = ov ? o : w_out - 1, xc = x0 + c0 + r;     // 32-bit offsets from uniform bases
    f16v acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    // operands of kMlpUnroll k-steps from input channel k0 on.  issue() only loads, from rows
    // clamped into the arrays; settle() zeroes what lies past a width just before the MFMAs.  The
    // empty asm pins each load ahead of its select, so the loads stay unconditional and in flight
    // together instead of sinking into one branch (and one wait) each.
    auto issue = [&](int k0, float (&a)[kMlpUnroll], float (&b)[kMlpUnroll]) {
#pragma unroll
        for (int u = 0; u < kMlpUnroll; ++u) {
            const int kr = k0 + 2 * u + h;
            const unsigned kc = kr < w_in ? kr : w_in - 1;
            a[u] = W[kc * w_out + wc];
            b[u] = mlp_lds[kc * tc + xc];
        }
    };
    auto settle = [&](int k0, float (&a)[kMlpUnroll], float (&b)[kMlpUnroll]) {
#pragma unroll
        for (int u = 0; u < kMlpUnroll; ++u) asm volatile("" : "+v"(a[u]), "+v"(b[u]));
#pragma unroll
        for (int u = 0; u < kMlpUnroll; ++u) {
            const bool kv = k0 + 2 * u + h < w_in;
            a[u] = (kv && ov) ? a[u] : 0.0f;
            b[u] = kv ? b[u] : 0.0f;
        }
    };
    auto mma = [&](const float (&a)[kMlpUnroll], const float (&b)[kMlpUnroll]) {
#pragma unroll
        for (int u = 0; u < kMlpUnroll; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
    };
    // two register sets: the loads of one group of k-steps are in flight under the MFMAs of the
    // group before it (the weights come from L2 or beyond)
    constexpr int kStep = 2 * kMlpUnroll;
    float a0[kMlpUnroll], b0[kMlpUnroll], a1[kMlpUnroll], b1[kMlpUnroll];
    issue(0, a0, b0);
#pragma nounroll
    for (int k0 = 0; k0 < w_in; k0 += 2 * kStep) {
        issue(k0 + kStep, a1, b1);
        settle(k0, a0, b0);
        mma(a0, b0);
        issue(k0 + 2 * kStep, a0, b0);
        settle(k0 + kStep, a1, b1);
        if (k0 + kStep < w_in) mma(a1, b1);
    }
    return acc;
}

}  // namespace
