// Which kernel computes the weight gradient of a dense convolution: one function of the call's shape, plain C++ without HIP or
// library state, so that tools/conv_wgrad_route_cases.cpp (tests/test_conv_wgrad_route_host.py) compiles it on the host.
// conv.hip fills the shape once per call (conv_wgrad_call), decides here and tells the launcher; the launchers do not ask again.
//
//   CW_DENSE_MM    dcn_wgrad_mm_kernel<NP, DENSE> (dcn_mm_kernels.h): grad_output pre-split once into MFMA fragment order, the
//                  regular grid as the sampling table
//   CW_PATCH       conv_wgrad_kernel (conv_wgrad_kernels.h): 3x3 / stride 1 / dilation 1, and 1x1 at any stride
//   CW_PATCH_JOBS  the same kernel with the jobs of lsn_conv2d_backward_weight_bn_jobs as its levels
//   CW_GENERAL     dcn_wgrad_xn_kernel<PLAIN> (dcn_kernels.h): every other validated shape; exact mode runs six products
#pragma once
#include <stdint.h>

enum ConvWgradRoute { CW_DENSE_MM, CW_PATCH, CW_PATCH_JOBS, CW_GENERAL };

constexpr int CW_MAXLV = 16;     // maps of one call (the kernels' own level tables are checked against it where they are filled)
constexpr int CW_STEP_PX = 32;   // pixels of one k-step of the fragment-order and general kernels (dcn.hip checks it is WG_BP)

struct ConvWgradLevel {
    int B, H, W, Ho, Wo;
    int P;   // B * Ho * Wo
};

struct ConvWgradShape {
    int n;   // levels; with fold_jobs > 1 they are the jobs
    ConvWgradLevel lv[CW_MAXLV];
    int C, Co, kh, kw, stride, dil;
    bool aligned16;       // every x and grad_out pointer
    int np, npl;          // bf16 products per product of the math mode (0: exact, 1, 3, 6) and its planes per operand
    bool general_gemms;   // LSN_DBG_GENERAL_GEMMS
    int fold_jobs;        // 0: a plain call; else the jobs of the folded norm
};

inline bool cw_below_2g(int64_t bytes) { return bytes < ((int64_t)1 << 31); }

// Whether the fragment-order kernel serves the shape (256 | Co, 64 | C, 16-byte aligned tensors at 32-bit byte offsets, a
// split-bf16 math mode) and is not slower than the patch kernel.
// Measured on the layer shapes of the benchmark step (tools/ubench/wgrad_ab.hip, profiles/r3_wgrad_ab.txt; batch 2): 3x3 at >= 4096
// output pixels 84 vs 96 us (layer 3), 262 vs 272 (FPN P3), 320 vs 380 (five head levels in one launch); 1x1 from >= 1024
// channels to >= 512: 75 vs 89, 53 vs 56; strided 1x1 from >= 512 channels: 83 vs 89, 78 vs 89.  Slower on the 1x1 layers
// with few input channels and many pixels (76 vs 52 us on 128 -> 512 at 100 x 168), which stay where they were.
inline bool cw_dense_mm_ok(const ConvWgradShape &s)
{
    if (s.Co % 256 != 0 || s.C % 64 != 0 || !s.aligned16 || s.np == 0 || s.general_gemms) return false;
    int64_t opx = 0, steps = 0;   // output pixels, 32-pixel k-steps
    for (int i = 0; i < s.n; ++i) {
        const ConvWgradLevel &L = s.lv[i];
        opx += L.P, steps += (L.P + CW_STEP_PX - 1) / CW_STEP_PX;
        if (!cw_below_2g((int64_t)L.B * L.H * L.W * s.C * 4) || !cw_below_2g((int64_t)L.P * s.Co * 4)) return false;
    }
    // (all of them measured at >= 2100 output pixels; smaller launches stay where they were)
    const bool win = s.kh * s.kw >= 9 ? opx >= 4096 : opx >= 2048 && ((s.C >= 1024 && s.Co >= 512) || (s.stride >= 2 && s.C >= 512));
    if (!win || steps < 8) return false;
    // the fragment image of grad_output at 32-bit byte offsets; the tap table: 2 GB
    return cw_below_2g(steps * 2 * (s.Co / 32) * s.npl * 1024) && opx * s.kh * s.kw < ((int64_t)1 << 26);
}

// (A strided 3x3 needs a 3 x 33 patch: one workgroup per CU and 2-way bank-conflicted tr-reads -- the general kernel was faster.)
inline bool cw_patch_ok(const ConvWgradShape &s)
{
    const bool k33 = s.kh == 3 && s.kw == 3 && s.stride == 1 && s.dil == 1, k11 = s.kh == 1 && s.kw == 1;
    if (!(k33 || k11) || s.n > CW_MAXLV || s.C % 4 != 0) return false;
    for (int i = 0; i < s.n; ++i)
        if (!cw_below_2g((int64_t)s.lv[i].B * s.lv[i].H * s.lv[i].W * s.C * 4) || !cw_below_2g((int64_t)s.lv[i].P * s.Co * 4)) return false;
    // (the narrow 3x3 form's 4 x 1 wave layout spills registers with one product per tap -- tools/kernel_resources.sh: 256
    // VGPRs + 7 .. 9 spilled -- so the one-product mode leaves those layers to the general kernel)
    if (k33 && s.Co <= 32) return s.np != 1;   // (the one configuration with guarded grad_output loads: any Co)
    return s.Co % 4 == 0;
}

// With fold_jobs > 1 the answer is CW_PATCH_JOBS or CW_GENERAL, and CW_GENERAL then says "no shared launch": the caller runs the
// jobs one by one, each routed as a call of its own.
inline ConvWgradRoute conv_wgrad_route(const ConvWgradShape &s)
{
    if (s.fold_jobs > 1) return (s.kh * s.kw * s.C) % 4 == 0 && cw_patch_ok(s) ? CW_PATCH_JOBS : CW_GENERAL;
    if (cw_dense_mm_ok(s)) return CW_DENSE_MM;
    return cw_patch_ok(s) ? CW_PATCH : CW_GENERAL;
}
