// Index, tie and divisor arithmetic of the pooling family (csrc/pool.hip: max / average pooling, the FPN's nearest
// upsample + add, corner pooling), written once for the device kernels and, compiled by a host compiler, for the loop-nest
// check of tests/test_pool_host.py against torch on the CPU.
//
// The rules are ATen's, so that the kernels return the bits the framework's operators return:
//   max pool      the window is walked in row-major order; a value takes over when it is greater than the running maximum
//                 (strict: the first maximum wins) or is a NaN (a NaN wins and stays until a later NaN replaces it);
//   average pool  output size and divisor of avg_pool2d with ceil_mode / count_include_pad; the window sum is divided by
//                 the divisor (a division, not a product with a reciprocal);
//   upsample      nearest-neighbour doubling: source index = destination index >> 1, for destination sizes 2h and 2h - 1;
//   corner pool   the running maximum of torch.cummax: a value takes over when it is >= the running maximum (the latest
//                 position in scan order wins a tie) or is a NaN; after a NaN only another NaN takes over.
#pragma once
#include <stdint.h>

#if !defined(LSN_HD)
#if defined(__HIPCC__)
#define LSN_HD __host__ __device__ __forceinline__
#else
#define LSN_HD static inline
#endif
#endif

// ---- windows -------------------------------------------------------------------------------------------------------
// Output extent of a pooling axis (ATen's pooling_output_shape): floor or ceiling of (in + 2 pad - k) / stride, plus 1; with
// ceil_mode a last window that would start in the right / bottom padding does not exist.  <= 0: no such pooling.
LSN_HD int pool_out_size(int in, int k, int stride, int pad, int ceil_mode)
{
    const int num = in + 2 * pad - k + (ceil_mode ? stride - 1 : 0);
    if (in <= 0 || k <= 0 || stride <= 0 || pad < 0 || num < 0) return 0;
    int o = num / stride + 1;
    if (ceil_mode && (o - 1) * stride >= in + pad) --o;
    return o;
}

// Window of output position o along one axis: its taps inside the image are [lo, hi); `ext` is its extent clipped to the
// padded image only (what count_include_pad counts).
LSN_HD void pool_window(int o, int k, int stride, int pad, int in, int *lo, int *hi, int *ext)
{
    const int start = o * stride - pad;
    const int end = start + k < in + pad ? start + k : in + pad;
    *ext = end - start;
    *lo = start > 0 ? start : 0;
    *hi = end < in ? end : in;
}

// Divisor of an average-pool window from the two axes' (lo, hi, ext)
LSN_HD int pool_avg_divisor(int hlo, int hhi, int hext, int wlo, int whi, int wext, int count_include_pad)
{
    return count_include_pad ? hext * wext : (hhi - hlo) * (whi - wlo);
}

// Output positions whose window covers input position i along one axis: [lo, hi], empty when lo > hi (gather-form backward)
LSN_HD void pool_cover(int i, int k, int stride, int pad, int out, int *lo, int *hi)
{
    const int a = i + pad - k + 1;                   // smallest start * stride that still reaches i
    *lo = a > 0 ? (a + stride - 1) / stride : 0;
    const int b = (i + pad) / stride;
    *hi = b < out - 1 ? b : out - 1;
}

// ---- max pool ------------------------------------------------------------------------------------------------------
LSN_HD int pool_max_takes(float v, float best) { return v > best || v != v; }

// ---- nearest upsample (x2) -------------------------------------------------------------------------------------------
LSN_HD int pool_up_ok(int small, int big) { return small > 0 && (big == 2 * small || big == 2 * small - 1); }
LSN_HD int pool_up_src(int dst) { return dst >> 1; }

// ---- corner pool -----------------------------------------------------------------------------------------------------
// mode: the border the maximum runs towards.  'top': out[y] = max over rows >= y, i.e. the scan starts at the bottom row.
enum { POOL_CORNER_TOP = 0, POOL_CORNER_BOTTOM = 1, POOL_CORNER_LEFT = 2, POOL_CORNER_RIGHT = 3 };

LSN_HD int pool_corner_along_x(int mode) { return mode >= POOL_CORNER_LEFT; }
// position along the scanned axis (n long) of scan step t
LSN_HD int pool_corner_pos(int mode, int t, int n) { return (mode == POOL_CORNER_TOP || mode == POOL_CORNER_LEFT) ? n - 1 - t : t; }
LSN_HD int pool_corner_takes(float v, float best) { return v != v || (best == best && v >= best); }
