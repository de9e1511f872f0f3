// Element arithmetic of the corner-point-verification targets and losses -- PointHMAssigner (lsnet_amd/core/assigners.py;
// reference: mmdet/core/bbox/assigners/point_hm_assigner.py:8-166) and GaussianFocalLoss / SmoothL1Loss / SEPFocalLoss
// (lsnet_amd/models/losses/cpv_losses.py), written once for the device kernels (csrc/cpv.hip) and, compiled by a host
// compiler, for the loop-nest check of tests/test_cpv_host.py.
//
// As in assign_rows.h every fp32 operation is rounded separately (no fused multiply-add): the host side is compiled with
// -ffp-contract=off, csrc/build.py compiles cpv.hip with it too, and products that feed a sum pass through assign_mul.
// expf / logf are the accurate library functions, never the fast intrinsics.
#pragma once
#include "assign_rows.h"

// ---- targets -------------------------------------------------------------------------------------------------------
// The constants gaussian_radius() forms from min_overlap in double precision before they meet an fp32 tensor.
struct cpv_radius_consts {
    float one_minus, one_plus;      // 1 - o, 1 + o
    float b3, c3;                   // -2 o, o - 1
    float four_a3, two_a3;          // 4 (4 o), 2 (4 o)
};

static inline cpv_radius_consts cpv_radius_constants(double min_overlap)
{
    cpv_radius_consts k;
    k.one_minus = (float)(1 - min_overlap), k.one_plus = (float)(1 + min_overlap);
    k.b3 = (float)(-2 * min_overlap), k.c3 = (float)(min_overlap - 1);
    k.four_a3 = (float)(4 * (4 * min_overlap)), k.two_a3 = (float)(2 * (4 * min_overlap));
    return k;
}

// CornerNet's radius of a (height, width) box: the minimum of the three cases, each term in the order of the statement
LSN_HD float cpv_gaussian_radius(float height, float width, const cpv_radius_consts &k)
{
    const float b1 = height + width;
    const float c1 = assign_mul(assign_mul(width, height), k.one_minus) / k.one_plus;
    const float r1 = (b1 - sqrtf(assign_mul(b1, b1) - assign_mul(4.f, c1))) / 2.f;
    const float b2 = assign_mul(2.f, height + width);
    const float c2 = assign_mul(assign_mul(k.one_minus, width), height);
    const float r2 = (b2 - sqrtf(assign_mul(b2, b2) - assign_mul(16.f, c2))) / 8.f;
    const float b3 = assign_mul(k.b3, height + width);
    const float c3 = assign_mul(assign_mul(k.c3, width), height);
    const float r3 = (b3 + sqrtf(assign_mul(b3, b3) - assign_mul(k.four_a3, c3))) / k.two_a3;
    return fminf(fminf(r1, r2), r3);
}

LSN_HD float cpv_sigma(float radius) { return (assign_mul(2.f, radius) + 1.f) / 6.f; }

// || xy - corner ||_2
LSN_HD float cpv_corner_distance(float px, float py, float cx, float cy)
{
    const float dx = px - cx, dy = py - cy;
    return sqrtf(assign_mul(dx, dx) + assign_mul(dy, dy));
}

// Gaussian of a point at distance d from a gt's corner; d >= radius is outside the bump (returns 0, as the statement's
// "no gt reaches this point")
LSN_HD float cpv_heat(float d, float radius, float sigma)
{
    if (d >= radius) return 0.f;
    return expf(-assign_mul(d, d) / assign_mul(assign_mul(2.f, sigma), sigma));
}

// sub-cell offset of a positive on FPN level `level`: (corner - xy) / 2^level
LSN_HD float cpv_offset(float corner, float xy, int level) { return (corner - xy) / (float)(1 << level); }

// levels a corner can be matched on: int(log2(stride)) in [0, CPV_LEVELS)
#define CPV_LEVELS 16

// ---- losses --------------------------------------------------------------------------------------------------------
LSN_HD float cpv_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// v^e: exponents 2 and 4 by multiplication, anything else by powf
LSN_HD float cpv_pow(float v, float e)
{
    if (e == 2.f) return v * v;
    if (e == 4.f) { const float s = v * v; return s * s; }
    return powf(v, e);
}

// d/dv v^e
LSN_HD float cpv_dpow(float v, float e)
{
    if (e == 2.f) return 2.f * v;
    if (e == 4.f) return 4.f * (v * v * v);
    return e * powf(v, e - 1.f);
}

// GaussianFocalLoss of one element on the LOGIT x against the heat-map target t (alpha: exponent of the probability terms,
// gamma: exponent of 1 - t):  pos = -log(p + eps) (1 - p)^alpha [t == 1],  neg = -log(1 - p + eps) p^alpha (1 - t)^gamma.
// -> the value; *dx: its derivative with respect to x.
LSN_HD float cpv_gaussian_focal(float x, float t, float alpha, float gamma, float *dx)
{
    const float eps = 1e-12f;
    const float p = cpv_sigmoid(x), q = 1.f - p;
    const float nw = cpv_pow(1.f - t, gamma);
    const float lq = logf(q + eps);
    float v = -lq * cpv_pow(p, alpha) * nw;
    // d/dp of the negative part: nw (p^alpha / (1 - p + eps) - log(1 - p + eps) alpha p^(alpha - 1))
    float dp = nw * (cpv_pow(p, alpha) / (q + eps) - lq * cpv_dpow(p, alpha));
    if (t == 1.f) {
        const float lp = logf(p + eps);
        v += -lp * cpv_pow(q, alpha);
        dp += -(cpv_pow(q, alpha) / (p + eps)) + lp * cpv_dpow(q, alpha);
    }
    if (dx) *dx = dp * (p * q);
    return v;
}

// SmoothL1Loss of one element: |d| < beta ? 0.5 d^2 / beta : |d| - 0.5 beta (strict), d = pred - target
LSN_HD float cpv_smooth_l1(float pred, float target, float beta, float *dpred)
{
    const float d = pred - target, a = fabsf(d);
    if (a < beta) {
        if (dpred) *dpred = d / beta;
        return 0.5f * a * a / beta;
    }
    if (dpred) *dpred = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    return a - 0.5f * beta;
}

// SEPFocalLoss element terms on the LOGIT x.  Positive (target == 1): -log(p) (1 - p)^gamma w alpha; negative (target < 1):
// -log(1 - p) p^gamma (1 - alpha).  Each -> the value, *dx the derivative with respect to x.
LSN_HD float cpv_sep_focal_pos(float x, float w, float gamma, float alpha, float *dx)
{
    const float p = cpv_sigmoid(x), q = 1.f - p, lp = logf(p);
    if (dx) *dx = (-(cpv_pow(q, gamma) / p) + lp * cpv_dpow(q, gamma)) * (p * q) * w * alpha;
    return -lp * cpv_pow(q, gamma) * w * alpha;
}

LSN_HD float cpv_sep_focal_neg(float x, float gamma, float alpha, float *dx)
{
    const float p = cpv_sigmoid(x), q = 1.f - p, lq = logf(q);
    if (dx) *dx = (cpv_pow(p, gamma) / q - lq * cpv_dpow(p, gamma)) * (p * q) * (1.f - alpha);
    return -lq * cpv_pow(p, gamma) * (1.f - alpha);
}

// source index of F.interpolate(mode='nearest') along one axis: the scale is formed in float as ATen forms it
LSN_HD int cpv_nearest_index(int dst, int in, int out)
{
    const float scale = (float)in / (float)out;
    const int s = (int)floorf((float)dst * scale);
    return s < in - 1 ? s : in - 1;
}
