// Row arithmetic of target assignment -- the per-(point, gt) and per-(box, gt) formulas of lsnet_amd/core/assigners.py
// (reference: mmdet/core/bbox/assigners/centroid_assigner.py:26-93, atss_assigner.py:29-164, iou2d_calculator.py:36-130),
// written once for the device kernels (csrc/assign.hip) and, compiled by a host compiler, for the loop-nest check of
// tests/test_assign_host.py.
//
// Every product and sum here is a separately rounded fp32 operation, as the elementwise torch statements round them:
// no fused multiply-add.  The host side is compiled with -ffp-contract=off; on the device every product that feeds an
// addition passes through an opaque register barrier (the library is built with -ffp-contract=fast, which ignores
// contraction pragmas), and csrc/build.py compiles assign.hip with -ffp-contract=off on top of that.  Division and
// square root are the correctly rounded ones (hipcc's default; never build this with fast-math).  log2f is glibc's on
// the host and the device library's in the kernel: both are exact at powers of two, where the truncation below could
// flip, and the strides are powers of two.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LSN_HD __host__ __device__ __forceinline__
#else
#define LSN_HD static inline
#endif

// a * b, rounded to fp32 before anything else uses it
LSN_HD float assign_mul(float a, float b)
{
    float p = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(p));
#endif
    return p;
}

// Unsigned key whose order is the ascending order of the floats; NaN is 0xffffffff, above everything (torch's order).
LSN_HD uint32_t assign_key(float v)
{
    union { float f; uint32_t u; } c;
    c.f = v;
    if (v != v) return 0xffffffffu;
    return (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
}

LSN_HD float assign_key_value(uint32_t key)
{
    union { float f; uint32_t u; } c;
    c.u = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
    return c.f;
}

// ---- ragged batches ----------------------------------------------------------------------------------------------
// Row i exists for the image whose mask row is `valid` (NULL: every row exists) -- the `inside` flags of a batch padded
// to its largest image.  A row that does not exist is never a candidate of that image's gts.
LSN_HD int assign_row_valid(const uint8_t *valid, size_t i) { return valid == 0 || valid[i] != 0; }

// The per-point targets LSHead builds from an assignment (lsnet_head.py:834-917: the targets of the filtered points,
// unmapped into the full grid with zeros).  gt_ind: 1-based gt of the image, num_gts: how many the image has.
LSN_HD int assign_target_positive(int64_t gt_ind, int valid, int num_gts) { return valid && gt_ind > 0 && gt_ind <= num_gts; }

// label of a point: its gt's label (1 without gt_labels), the background label where nothing was assigned, 0 outside the image
LSN_HD int64_t assign_target_label(int positive, int valid, const int64_t *image_gt_labels, int64_t gt_ind, int64_t background)
{
    if (!valid) return 0;
    if (!positive) return background;
    return image_gt_labels ? image_gt_labels[gt_ind - 1] : 1;
}

LSN_HD float assign_target_label_weight(int valid) { return valid ? 1.f : 0.f; }
LSN_HD float assign_target_bbox_weight(int positive) { return positive ? 1.f : 0.f; }
// column d of the point's target row: its gt's table row, zeros otherwise
LSN_HD float assign_target_value(int positive, const float *image_table, int D, int64_t gt_ind, int d)
{
    return positive ? image_table[(size_t)(gt_ind - 1) * D + d] : 0.f;
}

// ---- Centroid assigner -------------------------------------------------------------------------------------------
// FPN level of a point from its stride column: int(log2(stride)) (centroid_assigner.py:50)
LSN_HD int assign_point_level(float stride) { return (int)log2f(stride); }

// width / height of a gt, clamped as the assigner clamps them
LSN_HD float assign_gt_extent(float lo, float hi) { return fmaxf(hi - lo, 1e-6f); }

// level of a gt: int((log2(w / scale) + log2(h / scale)) / 2), clamped to the levels present among the points
LSN_HD int assign_gt_level(float w, float h, float scale, int lvl_min, int lvl_max)
{
    const int l = (int)((log2f(w / scale) + log2f(h / scale)) / 2.f);
    return l < lvl_min ? lvl_min : (l > lvl_max ? lvl_max : l);
}

LSN_HD float assign_box_centre(float lo, float hi) { return (lo + hi) / 2.f; }

// || (xy - centre) / wh ||_2
LSN_HD float assign_centroid_distance(float px, float py, float cx, float cy, float w, float h)
{
    const float dx = (px - cx) / w, dy = (py - cy) / h;
    return sqrtf(assign_mul(dx, dx) + assign_mul(dy, dy));
}

// ---- ATSS --------------------------------------------------------------------------------------------------------
// bbox_overlaps(mode='iou') of two xyxy boxes: overlap / max(area1 + area2 - overlap, 1e-6), no +1
LSN_HD float assign_iou(const float *b, const float *g)
{
    const float w = fmaxf(fminf(b[2], g[2]) - fmaxf(b[0], g[0]), 0.f);
    const float h = fmaxf(fminf(b[3], g[3]) - fmaxf(b[1], g[1]), 0.f);
    const float overlap = assign_mul(w, h);
    const float area1 = assign_mul(b[2] - b[0], b[3] - b[1]), area2 = assign_mul(g[2] - g[0], g[3] - g[1]);
    return overlap / fmaxf(area1 + area2 - overlap, 1e-6f);
}

// distance of two centres: sqrt(dx * dx + dy * dy)
LSN_HD float assign_centre_distance(float ax, float ay, float bx, float by)
{
    const float dx = ax - bx, dy = ay - by;
    return sqrtf(assign_mul(dx, dx) + assign_mul(dy, dy));
}

// a box centre lies inside a gt by more than 0.01 on every side
LSN_HD int assign_centre_inside(float cx, float cy, const float *g)
{
    return fminf(fminf(cx - g[0], cy - g[1]), fminf(g[2] - cx, g[3] - cy)) > 0.01f;
}

// mean + unbiased standard deviation (torch.std's default) of a gt's n candidate IoUs, summed in index order in two
// passes.  n == 1 gives NaN as torch does (0 / 0): nothing is >= NaN, the gt takes no box.
LSN_HD float assign_atss_threshold(const float *iou, int n)
{
    float sum = 0.f;
    for (int i = 0; i < n; ++i) sum += iou[i];
    const float mean = sum / (float)n;
    float sq = 0.f;
    for (int i = 0; i < n; ++i) {
        const float d = iou[i] - mean;
        sq += assign_mul(d, d);
    }
    return mean + sqrtf(sq / (float)(n - 1));
}
