// Element arithmetic of LSHead's point decoding (csrc/points.hip: softplus of the raw vector halves, their signed selection,
// the gradient_mul mix and base offsets that give the sampling offsets, the softplus of the refine sum, the proposal boxes of
// the refine-stage assignment), written once for the device kernels and, compiled by a host compiler, for the loop-nest check
// of tests/test_point_decode_host.py against torch on the CPU.
//
// Every statement keeps the rounding of the torch statement it replaces (models/dense_heads/ls_head.py): a product and the sum
// that follows it are rounded on their own, so the translation units that include this header are compiled with
// -ffp-contract=off.
//   softplus      nn.Softplus(beta 1, threshold 20): x > 20 ? x : log1pf(expf(x)); its derivative from the saved input as
//                 ATen's softplus_backward states it: z = expf(x), x > 20 ? g : g * z / (z + 1);
//   signed pair   (neg, pos) halves of a vector component -> pos if pos > neg else -neg (index 0 wins a tie and is negated:
//                 `_signed_pairs`); the gradient goes to the winner, negated for neg, and the loser gets 0;
//   mix           (1 - gm) * s.detach() + gm * s with 1 - gm formed in double and rounded to fp32 as the Python scalar is:
//                 fl(fl(one_minus * s) + fl(gm * s)), which is NOT s; only the second term carries a gradient, fl(gm * g);
//   boxes         extreme: [x of landmark 1, y of landmark 0, x of landmark 3, y of landmark 2] (`extreme_points2bbox`);
//                 vectors: [min x, min y, max x, max y] over the nv vectors, centre dropped (`vectors2bbox`);
//                 then point + fl(box * stride).
#pragma once
#include <math.h>
#include <stdint.h>

#if !defined(LSN_HD)
#if defined(__HIPCC__)
#define LSN_HD __host__ __device__ __forceinline__
#else
#define LSN_HD static inline
#endif
#endif

#define POINT_SOFTPLUS_THRESHOLD 20.0f

// ---- softplus --------------------------------------------------------------------------------------------------------
LSN_HD float point_softplus(float x) { return x > POINT_SOFTPLUS_THRESHOLD ? x : log1pf(expf(x)); }

// gradient g of softplus(x) -> gradient of x
LSN_HD float point_softplus_grad(float g, float x)
{
    const float z = expf(x);
    return x > POINT_SOFTPLUS_THRESHOLD ? g : g * z / (z + 1.0f);
}

// ---- signed pairs ----------------------------------------------------------------------------------------------------
LSN_HD int point_pos_wins(float neg, float pos) { return pos > neg; }
LSN_HD float point_signed(float neg, float pos) { return point_pos_wins(neg, pos) ? pos : -neg; }

// what the half `is_pos` (0: neg, 1: pos) of a pair receives of the gradient g_s of the signed value
LSN_HD float point_signed_grad(float g_s, float neg, float pos, int is_pos)
{
    const int win = point_pos_wins(neg, pos);
    if (is_pos) return win ? g_s : 0.0f;
    return win ? 0.0f : -g_s;
}

// ---- gradient_mul mix and base offset -----------------------------------------------------------------------------------
LSN_HD float point_one_minus(double gm) { return (float)(1.0 - gm); }

LSN_HD float point_offset(float s, float gm, float one_minus, float base)
{
    const float a = one_minus * s;
    const float b = gm * s;
    const float m = a + b;
    return m - base;
}

LSN_HD float point_offset_grad(float g_off, float gm) { return gm * g_off; }

// ---- the offset table ---------------------------------------------------------------------------------------------------
// Source of offset channel j: src >= 0 names the sp channel of the pair's neg half (pos is the next one); src < 0 names
// the free raw channel n_sp + (-1 - src).  Channel j = 2 t + comp (comp 0: y, 1: x) of a picked vector v reads the pair at
// 4 v + 2 comp.
LSN_HD int point_free_index(int src) { return -1 - src; }

// ---- proposal boxes -------------------------------------------------------------------------------------------------------
enum { POINT_BOX_EXTREME = 0, POINT_BOX_VECTORS = 1 };

// min / max that hand a NaN on, like torch.min / torch.max
LSN_HD float point_min(float a, float b) { return (b < a || b != b) ? b : a; }
LSN_HD float point_max(float a, float b) { return (b > a || b != b) ? b : a; }

// a row's vector v: its four halves [y_neg, y_pos, x_neg, x_pos] -> signed (y, x)
LSN_HD void point_vector_yx(const float *q, float *y, float *x)
{
    *y = point_signed(q[0], q[1]);
    *x = point_signed(q[2], q[3]);
}

LSN_HD float point_box_coord(float centre, float box, float stride)
{
    const float scaled = box * stride;
    return centre + scaled;
}
