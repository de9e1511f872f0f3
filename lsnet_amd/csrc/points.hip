// LSHead's point decoding in liblsnet_hip.so: the pixel-wise statements between the head's 1x1 outputs and their consumers
// (models/dense_heads/ls_head.py), one launch per pass instead of a dozen framework launches and their autograd chains:
//   point decode   raw init output -> sp = softplus(raw[:n_sp]) and the 2 x taps sampling offsets (signed selection of the
//                  picked vectors, free channels, gradient_mul mix, minus the base grid), forward and backward;
//   softplus-add   the refine stage's softplus(a + b) with b detached, forward and backward;
//   point boxes    the proposal boxes the refine-stage assignment reads, all levels and images in one launch.
// Arithmetic and its rounding: point_rows.h (this unit is compiled with -ffp-contract=off).
#include "common.h"
#include "point_rows.h"
#include "prof.h"

namespace lsn {

// ---------------------------------------------------------------------------------------------
// Streaming kernels over pixel rows (rows x C floats, every tensor with its own row pitch in floats, rows addressed with
// 64-bit offsets).  Lanes run along a row's channels first and along rows after that, so a wave touches whole rows.  V = 4:
// a lane moves four channels with one 16-byte access -- taken only when every pointer of the call is 16-byte aligned and
// every pitch and width a multiple of 4; V = 1 otherwise.  The 18-float offset rows are only 8-byte aligned from row to row:
// they are always accessed one float per lane (consecutive lanes, consecutive floats).
// Every output element is written by exactly one lane: no atomics, no workspace, the same bits on every run.
// ---------------------------------------------------------------------------------------------
constexpr int PT_THREADS = 256;
constexpr int PT_MAX_OFF = 32;      // offset channels (2 x taps; the head has 18)
constexpr int PT_MAX_RAW = 256;     // raw channels (the head has at most 4 * (36 + 1) = 148)
constexpr int PT_BOX_LANES = 16;    // lanes that share a row in the 'vectors' box mode

// src: point_rows.h's offset table; inv: its inverse over the raw channels -- for a softplus channel the offset channel that
// reads its pair, for a free channel the offset channel that copies it, -1 where there is none
struct PointTable {
    int n_off;
    int src[PT_MAX_OFF];
    short inv[PT_MAX_RAW];
};

__device__ __forceinline__ f32x4 pt_ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void pt_st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// item i of `total` = rows x per_row -> (row, item of the row).  A 64-bit division costs some hundred instructions and these
// kernels do little else per item: calls whose item count fits 31 bits -- all the head makes -- divide in 32 bits.
__device__ __forceinline__ void pt_split(long long i, int per_row, long long total, long long &r, int &k)
{
    if (total <= 0x7fffffffll) {
        const unsigned q = (unsigned)i / (unsigned)per_row;
        r = q, k = (int)((unsigned)i - q * (unsigned)per_row);
    } else {
        r = i / per_row, k = (int)(i - r * per_row);
    }
}

// ---- point decode ------------------------------------------------------------------------------------------------------
// Items of a row: n_sp / V softplus items, then n_off offset items.  An offset item evaluates the softplus of its pair again
// (the same function of the same input: the bits of the sp it would read back) instead of waiting for another lane's store.
template <int V>
__global__ __launch_bounds__(PT_THREADS) void point_decode_fwd_kernel(const float *__restrict__ raw, int raw_pitch, int n_sp,
                                                                      PointTable T, float gm, float one_minus,
                                                                      const float *__restrict__ base, float *__restrict__ sp,
                                                                      int sp_pitch, float *__restrict__ off, int off_pitch,
                                                                      long long rows)
{
    const int n_q = n_sp / V, per_row = n_q + T.n_off;
    const long long i = (long long)blockIdx.x * PT_THREADS + threadIdx.x;
    if (i >= rows * per_row) return;
    long long r;
    int k;
    pt_split(i, per_row, rows * per_row, r, k);
    const float *x = raw + r * raw_pitch;
    if (k < n_q) {
        float *dst = sp + r * sp_pitch + k * V;
        if (V == 4) {
            const f32x4 v = pt_ld4(x + k * 4);
            f32x4 y;
            y[0] = point_softplus(v[0]), y[1] = point_softplus(v[1]), y[2] = point_softplus(v[2]), y[3] = point_softplus(v[3]);
            pt_st4(dst, y);
        } else {
            *dst = point_softplus(x[k]);
        }
        return;
    }
    const int j = k - n_q, src = T.src[j];
    float s;
    if (src >= 0)
        s = point_signed(point_softplus(x[src]), point_softplus(x[src + 1]));
    else
        s = x[n_sp + point_free_index(src)];
    off[r * off_pitch + j] = point_offset(s, gm, one_minus, base[j]);
}

// Items of a row: c_raw / V.  g_sp / g_off may be NULL (no gradient reached that output).
template <int V>
__global__ __launch_bounds__(PT_THREADS) void point_decode_bwd_kernel(const float *__restrict__ raw, int raw_pitch, int c_raw,
                                                                      int n_sp, PointTable T, float gm,
                                                                      const float *__restrict__ sp, int sp_pitch,
                                                                      const float *__restrict__ g_sp, int gsp_pitch,
                                                                      const float *__restrict__ g_off, int goff_pitch,
                                                                      float *__restrict__ g_raw, int graw_pitch, long long rows)
{
    const int per_row = c_raw / V;
    const long long i = (long long)blockIdx.x * PT_THREADS + threadIdx.x;
    if (i >= rows * per_row) return;
    long long r;
    int c0;
    pt_split(i, per_row, rows * per_row, r, c0);
    c0 *= V;
    const float *x = raw + r * raw_pitch + c0;
    const float *go = g_off ? g_off + r * goff_pitch : nullptr;
    float xs[V], gs[V], out[V];
    const bool soft = c0 < n_sp;        // (n_sp and c0 are multiples of V: an item never straddles the two kinds)
    if (V == 4) {
        const f32x4 v = pt_ld4(x);
        xs[0] = v[0], xs[1] = v[1], xs[2] = v[2], xs[3] = v[3];
    } else {
        xs[0] = x[0];
    }
#pragma unroll
    for (int e = 0; e < V; ++e) gs[e] = 0.f;
    if (soft && g_sp) {
        const float *g = g_sp + r * gsp_pitch + c0;
        if (V == 4) {
            const f32x4 v = pt_ld4(g);
            gs[0] = v[0], gs[1] = v[1], gs[2] = v[2], gs[3] = v[3];
        } else {
            gs[0] = g[0];
        }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const int c = c0 + e, j = T.inv[c];
        if (!soft) {
            out[e] = (j >= 0 && go) ? point_offset_grad(go[j], gm) : 0.f;
            continue;
        }
        float g = gs[e];
        if (j >= 0 && go) {
            const float *pair = sp + r * sp_pitch + (c & ~1);
            g = g + point_signed_grad(point_offset_grad(go[j], gm), pair[0], pair[1], c & 1);
        }
        out[e] = point_softplus_grad(g, xs[e]);
    }
    float *dst = g_raw + r * graw_pitch + c0;
    if (V == 4) {
        const f32x4 v = {out[0], out[1], out[2], out[3]};
        pt_st4(dst, v);
    } else {
        *dst = out[0];
    }
}

// ---- softplus(a + b) ---------------------------------------------------------------------------------------------------
// BWD: y is the gradient of a (b is detached), g the gradient of the output; the sum is formed again from a and b
template <int V, bool BWD>
__global__ __launch_bounds__(PT_THREADS) void softplus_add_kernel(const float *__restrict__ a, int a_pitch,
                                                                  const float *__restrict__ b, int b_pitch,
                                                                  const float *__restrict__ g, int g_pitch, float *__restrict__ y,
                                                                  int y_pitch, int C, long long rows)
{
    const int per_row = C / V;
    const long long i = (long long)blockIdx.x * PT_THREADS + threadIdx.x;
    if (i >= rows * per_row) return;
    long long r;
    int c0;
    pt_split(i, per_row, rows * per_row, r, c0);
    c0 *= V;
    if (V == 4) {
        const f32x4 va = pt_ld4(a + r * a_pitch + c0), vb = pt_ld4(b + r * b_pitch + c0);
        f32x4 o;
        if (BWD) {
            const f32x4 vg = pt_ld4(g + r * g_pitch + c0);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = point_softplus_grad(vg[e], va[e] + vb[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = point_softplus(va[e] + vb[e]);
        }
        pt_st4(y + r * y_pitch + c0, o);
    } else {
        const float s = a[r * a_pitch + c0] + b[r * b_pitch + c0];
        y[r * y_pitch + c0] = BWD ? point_softplus_grad(g[r * g_pitch + c0], s) : point_softplus(s);
    }
}

// ---- proposal boxes ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pt_vector(const float *p, bool wide, float *y, float *x)
{
    float q[4];
    if (wide) {
        const f32x4 v = pt_ld4(p);
        q[0] = v[0], q[1] = v[1], q[2] = v[2], q[3] = v[3];
    } else {
        q[0] = p[0], q[1] = p[1], q[2] = p[2], q[3] = p[3];
    }
    point_vector_yx(q, y, x);
}

__device__ __forceinline__ void pt_box_store(float *dst, bool wide, const float *pt, float x0, float y0, float x1, float y1)
{
    const float px = pt[0], py = pt[1], s = pt[2];
    const f32x4 o = {point_box_coord(px, x0, s), point_box_coord(py, y0, s), point_box_coord(px, x1, s), point_box_coord(py, y1, s)};
    if (wide)
        pt_st4(dst, o);
    else
        dst[0] = o[0], dst[1] = o[1], dst[2] = o[2], dst[3] = o[3];
}

// one lane per row: landmarks 0..3 are the row's first 16 floats
__global__ __launch_bounds__(PT_THREADS) void point_boxes_extreme_kernel(const float *__restrict__ rows, int pitch,
                                                                         const float *__restrict__ points, int n_all,
                                                                         float *__restrict__ out, int out_pitch, long long n_rows,
                                                                         bool wide_in, bool wide_out)
{
    const long long r = (long long)blockIdx.x * PT_THREADS + threadIdx.x;
    if (r >= n_rows) return;
    const float *p = rows + r * pitch;
    float y[4], x[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) pt_vector(p + 4 * v, wide_in, &y[v], &x[v]);
    long long b;
    int n;
    pt_split(r, n_all, n_rows, b, n);
    pt_box_store(out + r * out_pitch, wide_out, points + n * 3, x[1], y[0], x[3], y[2]);
}

// PT_BOX_LANES lanes per row: lane l takes vectors l, l + 16, ...; minima and maxima meet by butterfly (exact in any order)
__global__ __launch_bounds__(PT_THREADS) void point_boxes_vectors_kernel(const float *__restrict__ rows, int pitch, int nv,
                                                                         const float *__restrict__ points, int n_all,
                                                                         float *__restrict__ out, int out_pitch, long long n_rows,
                                                                         bool wide_in, bool wide_out)
{
    const long long r_raw = ((long long)blockIdx.x * PT_THREADS + threadIdx.x) / PT_BOX_LANES;
    const int l = threadIdx.x % PT_BOX_LANES;
    const bool live = r_raw < n_rows;
    const long long r = live ? r_raw : n_rows - 1;      // (every lane of the wave takes part in the shuffles)
    const float *p = rows + r * pitch;
    const float inf = __builtin_inff();
    float x0 = inf, y0 = inf, x1 = -inf, y1 = -inf;
    for (int v = l; v < nv; v += PT_BOX_LANES) {
        float y, x;
        pt_vector(p + 4 * v, wide_in, &y, &x);
        x0 = point_min(x0, x), y0 = point_min(y0, y), x1 = point_max(x1, x), y1 = point_max(y1, y);
    }
#pragma unroll
    for (int m = PT_BOX_LANES / 2; m > 0; m >>= 1) {
        x0 = point_min(x0, __shfl_xor(x0, m, PT_BOX_LANES)), y0 = point_min(y0, __shfl_xor(y0, m, PT_BOX_LANES));
        x1 = point_max(x1, __shfl_xor(x1, m, PT_BOX_LANES)), y1 = point_max(y1, __shfl_xor(y1, m, PT_BOX_LANES));
    }
    if (live && l == 0) {
        long long b;
        int n;
        pt_split(r, n_all, n_rows, b, n);
        pt_box_store(out + r * out_pitch, wide_out, points + n * 3, x0, y0, x1, y1);
    }
}

// ---- argument checks -------------------------------------------------------------------------------------------------
static int check_rows(const char *what, const char *name, const void *p, int pitch, int width, bool may_be_null = false)
{
    if (p == nullptr && may_be_null) return 0;
    LSN_CHECK(p != nullptr, "%s: %s is NULL", what, name);
    LSN_CHECK(((uintptr_t)p & 3) == 0, "%s: %s is not 4-byte aligned", what, name);
    LSN_CHECK(pitch >= width, "%s: row pitch of %s is %d floats, below its width %d", what, name, pitch, width);
    return 0;
}

static inline bool wide_ok(const void *p, int pitch) { return p == nullptr || (((uintptr_t)p & 15) == 0 && pitch % 4 == 0); }

static int check_grid(const char *what, long long rows, int per_row, unsigned *blocks)
{
    LSN_CHECK(rows > 0, "%s: %lld rows", what, rows);
    const long long n = (rows * per_row + PT_THREADS - 1) / PT_THREADS;
    LSN_CHECK(rows < (1ll << 40) && n < (1ll << 31), "%s: %lld rows are too many for one call", what, rows);
    *blocks = (unsigned)n;
    return 0;
}

static int make_table(const char *what, PointTable &T, int c_raw, int n_sp, const int *src, int n_off)
{
    LSN_CHECK(src != nullptr, "%s: the offset table is NULL", what);
    LSN_CHECK(c_raw > 0 && c_raw <= PT_MAX_RAW, "%s: %d raw channels (1 .. %d)", what, c_raw, PT_MAX_RAW);
    LSN_CHECK(n_sp > 0 && n_sp <= c_raw && n_sp % 4 == 0, "%s: n_sp = %d is not a multiple of 4 in 4 .. c_raw = %d", what, n_sp, c_raw);
    LSN_CHECK(n_off > 0 && n_off <= PT_MAX_OFF, "%s: %d offset channels (1 .. %d)", what, n_off, PT_MAX_OFF);
    T.n_off = n_off;
    for (int c = 0; c < PT_MAX_RAW; ++c) T.inv[c] = -1;
    for (int j = 0; j < PT_MAX_OFF; ++j) T.src[j] = 0;
    for (int j = 0; j < n_off; ++j) {
        const int s = src[j];
        if (s >= 0) {
            LSN_CHECK(s % 2 == 0 && s + 1 < n_sp, "%s: offset channel %d picks the pair at %d outside the %d softplus channels", what, j,
                      s, n_sp);
            LSN_CHECK(T.inv[s] < 0, "%s: offset channels %d and %d pick the same pair at %d", what, (int)T.inv[s], j, s);
            T.inv[s] = T.inv[s + 1] = (short)j;
        } else {
            const int c = n_sp + point_free_index(s);
            LSN_CHECK(c >= n_sp && c < c_raw, "%s: offset channel %d picks free channel %d outside the row of %d", what, j,
                      point_free_index(s), c_raw);
            LSN_CHECK(T.inv[c] < 0, "%s: offset channels %d and %d pick the same free channel %d", what, (int)T.inv[c], j,
                      point_free_index(s));
            T.inv[c] = (short)j;
        }
        T.src[j] = s;
    }
    return 0;
}

}  // namespace lsn

using namespace lsn;

int lsn_point_decode_forward(const float *raw, int raw_pitch, int c_raw, int n_sp, const int *src, int n_off, double gradient_mul,
                             const float *base, float *sp, int sp_pitch, float *off, int off_pitch, int64_t rows,
                             lsn_stream_t stream)
{
    const char *what = "point decode forward";
    PointTable T;
    if (int rc = make_table(what, T, c_raw, n_sp, src, n_off)) return rc;
    if (int rc = check_rows(what, "raw", raw, raw_pitch, c_raw)) return rc;
    if (int rc = check_rows(what, "sp", sp, sp_pitch, n_sp)) return rc;
    if (int rc = check_rows(what, "off", off, off_pitch, n_off)) return rc;
    LSN_CHECK(base != nullptr, "%s: base is NULL", what);
    const bool wide = wide_ok(raw, raw_pitch) && wide_ok(sp, sp_pitch);
    unsigned blocks;
    if (int rc = check_grid(what, rows, n_sp / (wide ? 4 : 1) + n_off, &blocks)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const float one_minus = point_one_minus(gradient_mul);
    ProfSpan prof(PROF_POINTS, 0.0, 4.0 * rows * (c_raw + n_sp + n_off), st);
    if (wide)
        hipLaunchKernelGGL(point_decode_fwd_kernel<4>, dim3(blocks), dim3(PT_THREADS), 0, st, raw, raw_pitch, n_sp, T, (float)gradient_mul,
                           one_minus, base, sp, sp_pitch, off, off_pitch, (long long)rows);
    else
        hipLaunchKernelGGL(point_decode_fwd_kernel<1>, dim3(blocks), dim3(PT_THREADS), 0, st, raw, raw_pitch, n_sp, T, (float)gradient_mul,
                           one_minus, base, sp, sp_pitch, off, off_pitch, (long long)rows);
    LSN_HIP(hipGetLastError());
    return 0;
}

int lsn_point_decode_backward(const float *raw, int raw_pitch, int c_raw, int n_sp, const int *src, int n_off, double gradient_mul,
                              const float *sp, int sp_pitch, const float *g_sp, int gsp_pitch, const float *g_off, int goff_pitch,
                              float *g_raw, int graw_pitch, int64_t rows, lsn_stream_t stream)
{
    const char *what = "point decode backward";
    PointTable T;
    if (int rc = make_table(what, T, c_raw, n_sp, src, n_off)) return rc;
    if (int rc = check_rows(what, "raw", raw, raw_pitch, c_raw)) return rc;
    if (int rc = check_rows(what, "sp", sp, sp_pitch, n_sp)) return rc;
    if (int rc = check_rows(what, "g_sp", g_sp, gsp_pitch, n_sp, true)) return rc;
    if (int rc = check_rows(what, "g_off", g_off, goff_pitch, n_off, true)) return rc;
    if (int rc = check_rows(what, "g_raw", g_raw, graw_pitch, c_raw)) return rc;
    const bool wide = c_raw % 4 == 0 && wide_ok(raw, raw_pitch) && wide_ok(g_sp, gsp_pitch) && wide_ok(g_raw, graw_pitch);
    unsigned blocks;
    if (int rc = check_grid(what, rows, c_raw / (wide ? 4 : 1), &blocks)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfSpan prof(PROF_POINTS, 0.0, 4.0 * rows * (2 * c_raw + 2 * n_sp + n_off), st);
    if (wide)
        hipLaunchKernelGGL(point_decode_bwd_kernel<4>, dim3(blocks), dim3(PT_THREADS), 0, st, raw, raw_pitch, c_raw, n_sp, T,
                           (float)gradient_mul, sp, sp_pitch, g_sp, gsp_pitch, g_off, goff_pitch, g_raw, graw_pitch, (long long)rows);
    else
        hipLaunchKernelGGL(point_decode_bwd_kernel<1>, dim3(blocks), dim3(PT_THREADS), 0, st, raw, raw_pitch, c_raw, n_sp, T,
                           (float)gradient_mul, sp, sp_pitch, g_sp, gsp_pitch, g_off, goff_pitch, g_raw, graw_pitch, (long long)rows);
    LSN_HIP(hipGetLastError());
    return 0;
}

template <bool BWD>
static int softplus_add(const char *what, const float *a, int a_pitch, const float *b, int b_pitch, const float *g, int g_pitch,
                        float *y, int y_pitch, int C, int64_t rows, lsn_stream_t stream)
{
    LSN_CHECK(C > 0, "%s: C = %d", what, C);
    if (int rc = check_rows(what, "a", a, a_pitch, C)) return rc;
    if (int rc = check_rows(what, "b", b, b_pitch, C)) return rc;
    if (BWD)
        if (int rc = check_rows(what, "grad_y", g, g_pitch, C)) return rc;
    if (int rc = check_rows(what, BWD ? "grad_a" : "y", y, y_pitch, C)) return rc;
    const bool wide = C % 4 == 0 && wide_ok(a, a_pitch) && wide_ok(b, b_pitch) && wide_ok(g, g_pitch) && wide_ok(y, y_pitch);
    unsigned blocks;
    if (int rc = check_grid(what, rows, C / (wide ? 4 : 1), &blocks)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfSpan prof(PROF_POINTS, 0.0, 4.0 * rows * C * (BWD ? 4 : 3), st);
    if (wide)
        hipLaunchKernelGGL((softplus_add_kernel<4, BWD>), dim3(blocks), dim3(PT_THREADS), 0, st, a, a_pitch, b, b_pitch, g, g_pitch, y,
                           y_pitch, C, (long long)rows);
    else
        hipLaunchKernelGGL((softplus_add_kernel<1, BWD>), dim3(blocks), dim3(PT_THREADS), 0, st, a, a_pitch, b, b_pitch, g, g_pitch, y,
                           y_pitch, C, (long long)rows);
    LSN_HIP(hipGetLastError());
    return 0;
}

int lsn_softplus_add_forward(const float *a, int a_pitch, const float *b, int b_pitch, float *y, int y_pitch, int C, int64_t rows,
                             lsn_stream_t stream)
{
    return softplus_add<false>("softplus-add forward", a, a_pitch, b, b_pitch, nullptr, 0, y, y_pitch, C, rows, stream);
}

int lsn_softplus_add_backward(const float *a, int a_pitch, const float *b, int b_pitch, const float *grad_y, int gy_pitch,
                              float *grad_a, int ga_pitch, int C, int64_t rows, lsn_stream_t stream)
{
    return softplus_add<true>("softplus-add backward", a, a_pitch, b, b_pitch, grad_y, gy_pitch, grad_a, ga_pitch, C, rows, stream);
}

int lsn_point_boxes(const float *rows, int pitch, int C, const float *points, int n_all, int B, int mode, int nv, float *out,
                    int out_pitch, lsn_stream_t stream)
{
    const char *what = "point boxes";
    LSN_CHECK(mode == POINT_BOX_EXTREME || mode == POINT_BOX_VECTORS, "%s: mode %d (0 extreme, 1 vectors)", what, mode);
    LSN_CHECK(B > 0 && n_all > 0, "%s: B = %d, N = %d", what, B, n_all);
    LSN_CHECK(points != nullptr, "%s: points is NULL", what);
    const int need = mode == POINT_BOX_EXTREME ? 16 : 4 * nv;
    LSN_CHECK(nv > 0 && C >= need, "%s: mode %d with %d vectors reads %d channels of a row of %d", what, mode, nv, need, C);
    if (int rc = check_rows(what, "rows", rows, pitch, C)) return rc;
    if (int rc = check_rows(what, "out", out, out_pitch, 4)) return rc;
    const long long n_rows = (long long)B * n_all;
    unsigned blocks;
    if (int rc = check_grid(what, n_rows, mode == POINT_BOX_EXTREME ? 1 : PT_BOX_LANES, &blocks)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool wide_in = wide_ok(rows, pitch), wide_out = wide_ok(out, out_pitch);
    ProfSpan prof(PROF_POINTS, 0.0, 4.0 * n_rows * (need + 4), st);
    if (mode == POINT_BOX_EXTREME)
        hipLaunchKernelGGL(point_boxes_extreme_kernel, dim3(blocks), dim3(PT_THREADS), 0, st, rows, pitch, points, n_all, out,
                           out_pitch, n_rows, wide_in, wide_out);
    else
        hipLaunchKernelGGL(point_boxes_vectors_kernel, dim3(blocks), dim3(PT_THREADS), 0, st, rows, pitch, nv, points, n_all, out,
                           out_pitch, n_rows, wide_in, wide_out);
    LSN_HIP(hipGetLastError());
    return 0;
}
