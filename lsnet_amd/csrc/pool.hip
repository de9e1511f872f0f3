// The pooling / resampling family of liblsnet_hip.so: max pool (ResNet stem, FPN extra levels), average pool (Res2Net),
// nearest upsample + add (FPN top-down pathway) and corner pool (corner-point-verification head), forward and backward.
#include "common.h"
#include "pool_rows.h"

namespace lsn {

// ---------------------------------------------------------------------------------------------
// Streaming kernels, bound by memory traffic.  All tensors are fp32 channels-last: pixel rows of C floats, each tensor with
// its own pixel pitch in floats (a channel slice of a wider tensor is read, a slot of a wider one written, in place); image
// b of an (H, W) map starts at b * H * W * pitch.  One lane owns 4 consecutive channels of one pixel (one line for the
// corner pool) and moves them with 16-byte loads and stores; consecutive lanes take consecutive channel quads, then
// consecutive pixels, so a wave touches whole pixel rows.
// Every backward is in gather form: a lane sums the gradients that reach its own pixel in a fixed order and stores once.
// No atomics, no workspace.  Index, tie and divisor rules: pool_rows.h.
// ---------------------------------------------------------------------------------------------
constexpr int POOL_THREADS = 256;

struct PoolGeom {
    int B, H, W, Ho, Wo, CQ;        // input map, output map, channel quads
    int kh, kw, stride, pad;
    int ceil_mode, count_include_pad;
};

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// lane -> (channel quad, x, y, image) of a (B, h, w, CQ) grid; false past its end
__device__ __forceinline__ bool pool_lane(int h, int w, int cq_n, int total, int &cq, int &x, int &y, int &b)
{
    const int i = blockIdx.x * POOL_THREADS + threadIdx.x;
    if (i >= total) return false;
    cq = i % cq_n;
    const int p = i / cq_n;
    x = p % w;
    const int r = p / w;
    y = r % h;
    b = r / h;
    return true;
}

__device__ __forceinline__ size_t pool_px(int b, int y, int x, int h, int w, int pitch)
{
    return (((size_t)b * h + y) * w + x) * (size_t)pitch;
}

// ---- max pool ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(POOL_THREADS) void max_pool_fwd_kernel(const float *__restrict__ x, int xp, float *__restrict__ y,
                                                                    int yp, uint8_t *__restrict__ slot, PoolGeom g, int total)
{
    int cq, ow, oh, b;
    if (!pool_lane(g.Ho, g.Wo, g.CQ, total, cq, ow, oh, b)) return;
    const int h0 = oh * g.stride - g.pad, w0 = ow * g.stride - g.pad;
    const int ilo = h0 < 0 ? -h0 : 0, ihi = h0 + g.kh > g.H ? g.H - h0 : g.kh;
    const int jlo = w0 < 0 ? -w0 : 0, jhi = w0 + g.kw > g.W ? g.W - w0 : g.kw;
    const float ninf = -__builtin_inff();
    f32x4 best = {ninf, ninf, ninf, ninf};
    const int first = ilo * g.kw + jlo;         // (a window of -inf only names its first tap, as ATen does)
    int s0 = first, s1 = first, s2 = first, s3 = first;
    for (int i = ilo; i < ihi; ++i)
        for (int j = jlo; j < jhi; ++j) {
            const f32x4 v = ld4(x + pool_px(b, h0 + i, w0 + j, g.H, g.W, xp) + cq * 4);
            const int s = i * g.kw + j;
            if (pool_max_takes(v[0], best[0])) best[0] = v[0], s0 = s;
            if (pool_max_takes(v[1], best[1])) best[1] = v[1], s1 = s;
            if (pool_max_takes(v[2], best[2])) best[2] = v[2], s2 = s;
            if (pool_max_takes(v[3], best[3])) best[3] = v[3], s3 = s;
        }
    st4(y + pool_px(b, oh, ow, g.Ho, g.Wo, yp) + cq * 4, best);
    if (slot) {
        const unsigned packed = (unsigned)s0 | (unsigned)s1 << 8 | (unsigned)s2 << 16 | (unsigned)s3 << 24;
        *reinterpret_cast<unsigned *>(slot + pool_px(b, oh, ow, g.Ho, g.Wo, g.CQ * 4) + cq * 4) = packed;
    }
}

// slot == nullptr: a 1 x 1 window, every covering output names the pixel
__global__ __launch_bounds__(POOL_THREADS) void max_pool_bwd_kernel(const float *__restrict__ gy, int gyp,
                                                                    const uint8_t *__restrict__ slot, float *__restrict__ gx,
                                                                    int gxp, PoolGeom g, int total)
{
    int cq, iw, ih, b;
    if (!pool_lane(g.H, g.W, g.CQ, total, cq, iw, ih, b)) return;
    int olo, ohi, plo, phi;
    pool_cover(ih, g.kh, g.stride, g.pad, g.Ho, &olo, &ohi);
    pool_cover(iw, g.kw, g.stride, g.pad, g.Wo, &plo, &phi);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int oh = olo; oh <= ohi; ++oh)
        for (int ow = plo; ow <= phi; ++ow) {
            const f32x4 d = ld4(gy + pool_px(b, oh, ow, g.Ho, g.Wo, gyp) + cq * 4);
            if (slot) {
                const unsigned mine = (unsigned)((ih - (oh * g.stride - g.pad)) * g.kw + (iw - (ow * g.stride - g.pad)));
                const unsigned s = *reinterpret_cast<const unsigned *>(slot + pool_px(b, oh, ow, g.Ho, g.Wo, g.CQ * 4) + cq * 4);
                if ((s & 0xffu) == mine) acc[0] += d[0];
                if ((s >> 8 & 0xffu) == mine) acc[1] += d[1];
                if ((s >> 16 & 0xffu) == mine) acc[2] += d[2];
                if ((s >> 24) == mine) acc[3] += d[3];
            } else {
                acc += d;
            }
        }
    st4(gx + pool_px(b, ih, iw, g.H, g.W, gxp) + cq * 4, acc);
}

// ---- average pool --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(POOL_THREADS) void avg_pool_fwd_kernel(const float *__restrict__ x, int xp, float *__restrict__ y,
                                                                    int yp, PoolGeom g, int total)
{
    int cq, ow, oh, b;
    if (!pool_lane(g.Ho, g.Wo, g.CQ, total, cq, ow, oh, b)) return;
    int hlo, hhi, hext, wlo, whi, wext;
    pool_window(oh, g.kh, g.stride, g.pad, g.H, &hlo, &hhi, &hext);
    pool_window(ow, g.kw, g.stride, g.pad, g.W, &wlo, &whi, &wext);
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    for (int ih = hlo; ih < hhi; ++ih)
        for (int iw = wlo; iw < whi; ++iw) sum += ld4(x + pool_px(b, ih, iw, g.H, g.W, xp) + cq * 4);
    if (hlo < hhi && wlo < whi) {
        const float div = (float)pool_avg_divisor(hlo, hhi, hext, wlo, whi, wext, g.count_include_pad);
        sum[0] /= div, sum[1] /= div, sum[2] /= div, sum[3] /= div;
    }
    st4(y + pool_px(b, oh, ow, g.Ho, g.Wo, yp) + cq * 4, sum);
}

__global__ __launch_bounds__(POOL_THREADS) void avg_pool_bwd_kernel(const float *__restrict__ gy, int gyp, float *__restrict__ gx,
                                                                    int gxp, PoolGeom g, int total)
{
    int cq, iw, ih, b;
    if (!pool_lane(g.H, g.W, g.CQ, total, cq, iw, ih, b)) return;
    int olo, ohi, plo, phi;
    pool_cover(ih, g.kh, g.stride, g.pad, g.Ho, &olo, &ohi);
    pool_cover(iw, g.kw, g.stride, g.pad, g.Wo, &plo, &phi);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int oh = olo; oh <= ohi; ++oh) {
        int hlo, hhi, hext;
        pool_window(oh, g.kh, g.stride, g.pad, g.H, &hlo, &hhi, &hext);
        for (int ow = plo; ow <= phi; ++ow) {
            int wlo, whi, wext;
            pool_window(ow, g.kw, g.stride, g.pad, g.W, &wlo, &whi, &wext);
            const float div = (float)pool_avg_divisor(hlo, hhi, hext, wlo, whi, wext, g.count_include_pad);
            const f32x4 d = ld4(gy + pool_px(b, oh, ow, g.Ho, g.Wo, gyp) + cq * 4);
            acc[0] += d[0] / div, acc[1] += d[1] / div, acc[2] += d[2] / div, acc[3] += d[3] / div;
        }
    }
    st4(gx + pool_px(b, ih, iw, g.H, g.W, gxp) + cq * 4, acc);
}

// ---- nearest upsample + add ------------------------------------------------------------------------------------------
// out may be lat itself: a lane reads and writes the same 16 bytes
__global__ __launch_bounds__(POOL_THREADS) void upsample_add_fwd_kernel(const float *__restrict__ top, int tp, const float *lat,
                                                                        int lp, float *out, int op, int h, int w, int H, int W,
                                                                        int CQ, int total)
{
    int cq, x, y, b;
    if (!pool_lane(H, W, CQ, total, cq, x, y, b)) return;
    const f32x4 t = ld4(top + pool_px(b, pool_up_src(y), pool_up_src(x), h, w, tp) + cq * 4);
    const f32x4 l = ld4(lat + pool_px(b, y, x, H, W, lp) + cq * 4);
    st4(out + pool_px(b, y, x, H, W, op) + cq * 4, l + t);
}

template <bool ACC>
__global__ __launch_bounds__(POOL_THREADS) void upsample_add_bwd_kernel(const float *__restrict__ go, int gp, float *__restrict__ gt,
                                                                        int tp, int h, int w, int H, int W, int CQ, int total)
{
    int cq, x, y, b;
    if (!pool_lane(h, w, CQ, total, cq, x, y, b)) return;
    const bool right = 2 * x + 1 < W, down = 2 * y + 1 < H;
    f32x4 acc = ld4(go + pool_px(b, 2 * y, 2 * x, H, W, gp) + cq * 4);
    if (right) acc += ld4(go + pool_px(b, 2 * y, 2 * x + 1, H, W, gp) + cq * 4);
    if (down) acc += ld4(go + pool_px(b, 2 * y + 1, 2 * x, H, W, gp) + cq * 4);
    if (right && down) acc += ld4(go + pool_px(b, 2 * y + 1, 2 * x + 1, H, W, gp) + cq * 4);
    float *dst = gt + pool_px(b, y, x, h, w, tp) + cq * 4;
    if (ACC) acc = ld4(dst) + acc;
    st4(dst, acc);
}

// ---- corner pool -----------------------------------------------------------------------------------------------------
// A lane owns a channel quad of one line (a column for top / bottom, a row for left / right) and walks it in scan order.  The
// largest map of the verification head has some 5 000 such lanes, far fewer than the device holds: the walk is bound by memory
// latency, not bandwidth, so a walk issues the loads of eight steps together, before the first comparison of the chunk (only
// the comparisons depend on each other).
struct CornerLine {
    size_t base;      // pixel index of scan step 0 (times the pitch: its address)
    long long step;   // pixels from one scan step to the next (negative for top / left)
    int n;
};

__device__ __forceinline__ bool corner_line(int mode, int B, int H, int W, int CQ, int &cq, CornerLine &ln)
{
    const bool along_x = pool_corner_along_x(mode);
    const int lines = along_x ? H : W, total = B * lines * CQ;
    const int i = blockIdx.x * POOL_THREADS + threadIdx.x;
    if (i >= total) return false;
    cq = i % CQ;
    const int l = (i / CQ) % lines, b = i / CQ / lines;
    ln.n = along_x ? W : H;
    const int p0 = pool_corner_pos(mode, 0, ln.n), p1 = ln.n > 1 ? pool_corner_pos(mode, 1, ln.n) : p0;
    ln.base = along_x ? ((size_t)b * H + l) * W + p0 : ((size_t)b * H + p0) * W + l;
    ln.step = (long long)(p1 - p0) * (along_x ? 1 : W);
    return true;
}

// steps whose loads are issued together, before the first comparison of the chunk
constexpr int CORNER_CHUNK = 8;
// the value is in its registers here: keeps the compiler from moving a chunk's loads down to their uses, one round trip each
__device__ __forceinline__ void corner_pin(f32x4 &v) { asm volatile("" : "+v"(v)); }

template <bool ACC>
__global__ __launch_bounds__(POOL_THREADS) void corner_pool_fwd_kernel(int mode, const float *__restrict__ x, int xp,
                                                                       float *__restrict__ y, int yp, int B, int H, int W, int CQ)
{
    int cq;
    CornerLine ln;
    if (!corner_line(mode, B, H, W, CQ, cq, ln)) return;
    const float *xs = x + ln.base * xp + cq * 4;
    float *ys = y + ln.base * yp + cq * 4;
    const long long xstep = ln.step * xp, ystep = ln.step * yp;
    f32x4 best = ld4(xs);
    for (int t0 = 0; t0 < ln.n; t0 += CORNER_CHUNK) {
        f32x4 v[CORNER_CHUNK], o[CORNER_CHUNK];
#pragma unroll
        for (int k = 0; k < CORNER_CHUNK; ++k) {
            const int t = t0 + k < ln.n ? t0 + k : ln.n - 1;      // (past the end: the last step again, not used)
            v[k] = ld4(xs + t * xstep);
            if (ACC) o[k] = ld4(ys + t * ystep);
        }
#pragma unroll
        for (int k = 0; k < CORNER_CHUNK; ++k) {
            corner_pin(v[k]);
            if (ACC) corner_pin(o[k]);
        }
#pragma unroll
        for (int k = 0; k < CORNER_CHUNK; ++k) {
            if (t0 + k >= ln.n) break;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (pool_corner_takes(v[k][c], best[c])) best[c] = v[k][c];
            st4(ys + (t0 + k) * ystep, ACC ? o[k] + best : best);
        }
    }
}

// The output positions that share an argmax are a contiguous run of the scan: their gradients are summed in scan order and
// stored once, at the argmax, when the next run begins; every other position of the line gets 0 (nothing, when accumulating).
// A step first clears its own position (one 16-byte store); the four channels of the quad carry a run each, and the store
// that ends a run is a single float at the run's argmax -- rare: a line has few new maxima.  A lane's stores to one address
// stay in program order, so the sum lands on the cleared position.
template <bool ACC>
__global__ __launch_bounds__(POOL_THREADS) void corner_pool_bwd_kernel(int mode, const float *__restrict__ x, int xp,
                                                                       const float *__restrict__ gy, int gyp,
                                                                       float *__restrict__ gx, int gxp, int B, int H, int W, int CQ)
{
    int cq;
    CornerLine ln;
    if (!corner_line(mode, B, H, W, CQ, cq, ln)) return;
    const float *xs = x + ln.base * xp + cq * 4;
    const float *gs = gy + ln.base * gyp + cq * 4;
    float *ds = gx + ln.base * gxp + cq * 4;
    const long long xstep = ln.step * xp, gstep = ln.step * gyp, dstep = ln.step * gxp;
    f32x4 best = ld4(xs), acc = {0.f, 0.f, 0.f, 0.f};
    int pos[4] = {0, 0, 0, 0};
    for (int t0 = 0; t0 < ln.n; t0 += CORNER_CHUNK) {
        f32x4 v[CORNER_CHUNK], d[CORNER_CHUNK];
#pragma unroll
        for (int k = 0; k < CORNER_CHUNK; ++k) {
            const int t = t0 + k < ln.n ? t0 + k : ln.n - 1;
            v[k] = ld4(xs + t * xstep);
            d[k] = ld4(gs + t * gstep);
        }
#pragma unroll
        for (int k = 0; k < CORNER_CHUNK; ++k) corner_pin(v[k]), corner_pin(d[k]);
#pragma unroll
        for (int k = 0; k < CORNER_CHUNK; ++k) {
            const int t = t0 + k;
            if (t >= ln.n) break;
            if (!ACC) {
                float *here = ds + t * dstep;
                here[0] = 0.f, here[1] = 0.f, here[2] = 0.f, here[3] = 0.f;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (pool_corner_takes(v[k][c], best[c])) {
                    if (t > 0) {
                        float *dst = ds + pos[c] * dstep + c;
                        *dst = ACC ? *dst + acc[c] : acc[c];
                    }
                    best[c] = v[k][c], pos[c] = t, acc[c] = d[k][c];
                } else {
                    acc[c] += d[k][c];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float *dst = ds + pos[c] * dstep + c;
        *dst = ACC ? *dst + acc[c] : acc[c];
    }
}

// ---- argument checks -------------------------------------------------------------------------------------------------
static int check_tensor(const char *what, const char *name, const void *p, int pitch, int C)
{
    LSN_CHECK(p != nullptr, "%s: %s is NULL", what, name);
    LSN_CHECK(pitch >= C && pitch % 4 == 0, "%s: pixel pitch of %s is %d floats (a multiple of 4, at least C = %d)", what, name,
              pitch, C);
    LSN_CHECK(((uintptr_t)p & 15) == 0, "%s: %s is not 16-byte aligned", what, name);
    return 0;
}

static int check_map(const char *what, int B, int H, int W, int C)
{
    LSN_CHECK(B > 0 && H > 0 && W > 0 && C > 0, "%s: B = %d, H = %d, W = %d, C = %d", what, B, H, W, C);
    LSN_CHECK(C % 4 == 0, "%s: C = %d is not a multiple of 4", what, C);
    LSN_CHECK((long long)B * H * W * (C / 4) < (1ll << 31), "%s: %d x %d x %d x %d is too large for one call", what, B, H, W, C);
    return 0;
}

static int make_geom(const char *what, PoolGeom &g, int B, int H, int W, int C, int kh, int kw, int stride, int pad, int ceil_mode,
                     int count_include_pad)
{
    if (int rc = check_map(what, B, H, W, C)) return rc;
    LSN_CHECK(kh > 0 && kw > 0 && kh * kw <= 255 && stride > 0, "%s: window %d x %d, stride %d", what, kh, kw, stride);
    LSN_CHECK(pad >= 0 && 2 * pad <= kh && 2 * pad <= kw, "%s: pad %d should be at most half of the window %d x %d", what, pad, kh, kw);
    g.B = B, g.H = H, g.W = W, g.CQ = C / 4;
    g.kh = kh, g.kw = kw, g.stride = stride, g.pad = pad, g.ceil_mode = ceil_mode != 0, g.count_include_pad = count_include_pad != 0;
    g.Ho = pool_out_size(H, kh, stride, pad, g.ceil_mode), g.Wo = pool_out_size(W, kw, stride, pad, g.ceil_mode);
    LSN_CHECK(g.Ho > 0 && g.Wo > 0, "%s: a %d x %d map has no %d x %d window (pad %d)", what, H, W, kh, kw, pad);
    return 0;
}

static inline dim3 pool_grid(int total) { return dim3((unsigned)cdiv(total, POOL_THREADS)); }

static int check_corner(const char *what, int mode, int B, int H, int W, int C)
{
    LSN_CHECK(mode >= POOL_CORNER_TOP && mode <= POOL_CORNER_RIGHT, "%s: mode %d (0 top, 1 bottom, 2 left, 3 right)", what, mode);
    return check_map(what, B, H, W, C);
}

static int check_up(const char *what, int B, int h, int w, int H, int W, int C)
{
    if (int rc = check_map(what, B, H, W, C)) return rc;
    LSN_CHECK(pool_up_ok(h, H) && pool_up_ok(w, W), "%s: %d x %d -> %d x %d is not a doubling (2n or 2n - 1 per axis)", what, h, w, H,
              W);
    return 0;
}

}  // namespace lsn

using namespace lsn;

int lsn_pool_output_size(int in, int k, int stride, int pad, int ceil_mode)
{
    return pool_out_size(in, k, stride, pad, ceil_mode != 0);
}

int lsn_max_pool2d_forward(const float *x, int x_pitch, float *y, int y_pitch, uint8_t *slot, int B, int H, int W, int C, int kh,
                           int kw, int stride, int pad, lsn_stream_t stream)
{
    const char *what = "max pool forward";
    PoolGeom g;
    if (int rc = make_geom(what, g, B, H, W, C, kh, kw, stride, pad, 0, 0)) return rc;
    if (int rc = check_tensor(what, "x", x, x_pitch, C)) return rc;
    if (int rc = check_tensor(what, "y", y, y_pitch, C)) return rc;
    LSN_CHECK(((uintptr_t)slot & 3) == 0, "%s: slot is not 4-byte aligned", what);
    const int total = B * g.Ho * g.Wo * g.CQ;
    hipLaunchKernelGGL(max_pool_fwd_kernel, pool_grid(total), dim3(POOL_THREADS), 0, stream, x, x_pitch, y, y_pitch, slot, g, total);
    LSN_HIP(hipGetLastError());
    return 0;
}

int lsn_max_pool2d_backward(const float *grad_y, int gy_pitch, const uint8_t *slot, float *grad_x, int gx_pitch, int B, int H, int W,
                            int C, int kh, int kw, int stride, int pad, lsn_stream_t stream)
{
    const char *what = "max pool backward";
    PoolGeom g;
    if (int rc = make_geom(what, g, B, H, W, C, kh, kw, stride, pad, 0, 0)) return rc;
    if (int rc = check_tensor(what, "grad_y", grad_y, gy_pitch, C)) return rc;
    if (int rc = check_tensor(what, "grad_x", grad_x, gx_pitch, C)) return rc;
    LSN_CHECK(slot != nullptr || kh * kw == 1, "%s: a %d x %d window needs the slots of the forward", what, kh, kw);
    LSN_CHECK(((uintptr_t)slot & 3) == 0, "%s: slot is not 4-byte aligned", what);
    const int total = B * H * W * g.CQ;
    hipLaunchKernelGGL(max_pool_bwd_kernel, pool_grid(total), dim3(POOL_THREADS), 0, stream, grad_y, gy_pitch, slot, grad_x, gx_pitch,
                       g, total);
    LSN_HIP(hipGetLastError());
    return 0;
}

int lsn_avg_pool2d_forward(const float *x, int x_pitch, float *y, int y_pitch, int B, int H, int W, int C, int kh, int kw, int stride,
                           int pad, int ceil_mode, int count_include_pad, lsn_stream_t stream)
{
    const char *what = "avg pool forward";
    PoolGeom g;
    if (int rc = make_geom(what, g, B, H, W, C, kh, kw, stride, pad, ceil_mode, count_include_pad)) return rc;
    if (int rc = check_tensor(what, "x", x, x_pitch, C)) return rc;
    if (int rc = check_tensor(what, "y", y, y_pitch, C)) return rc;
    const int total = B * g.Ho * g.Wo * g.CQ;
    hipLaunchKernelGGL(avg_pool_fwd_kernel, pool_grid(total), dim3(POOL_THREADS), 0, stream, x, x_pitch, y, y_pitch, g, total);
    LSN_HIP(hipGetLastError());
    return 0;
}

int lsn_avg_pool2d_backward(const float *grad_y, int gy_pitch, float *grad_x, int gx_pitch, int B, int H, int W, int C, int kh, int kw,
                            int stride, int pad, int ceil_mode, int count_include_pad, lsn_stream_t stream)
{
    const char *what = "avg pool backward";
    PoolGeom g;
    if (int rc = make_geom(what, g, B, H, W, C, kh, kw, stride, pad, ceil_mode, count_include_pad)) return rc;
    if (int rc = check_tensor(what, "grad_y", grad_y, gy_pitch, C)) return rc;
    if (int rc = check_tensor(what, "grad_x", grad_x, gx_pitch, C)) return rc;
    const int total = B * H * W * g.CQ;
    hipLaunchKernelGGL(avg_pool_bwd_kernel, pool_grid(total), dim3(POOL_THREADS), 0, stream, grad_y, gy_pitch, grad_x, gx_pitch, g,
                       total);
    LSN_HIP(hipGetLastError());
    return 0;
}

int lsn_upsample_add_forward(const float *top, int top_pitch, const float *lat, int lat_pitch, float *out, int out_pitch, int B, int h,
                             int w, int H, int W, int C, lsn_stream_t stream)
{
    const char *what = "upsample-add forward";
    if (int rc = check_up(what, B, h, w, H, W, C)) return rc;
    if (int rc = check_tensor(what, "top", top, top_pitch, C)) return rc;
    if (int rc = check_tensor(what, "lat", lat, lat_pitch, C)) return rc;
    if (int rc = check_tensor(what, "out", out, out_pitch, C)) return rc;
    LSN_CHECK(out != lat || out_pitch == lat_pitch, "%s: out aliases lat with another pitch", what);
    const int total = B * H * W * (C / 4);
    hipLaunchKernelGGL(upsample_add_fwd_kernel, pool_grid(total), dim3(POOL_THREADS), 0, stream, top, top_pitch, lat, lat_pitch, out,
                       out_pitch, h, w, H, W, C / 4, total);
    LSN_HIP(hipGetLastError());
    return 0;
}

int lsn_upsample_add_backward(const float *grad_out, int go_pitch, float *grad_top, int gt_pitch, int accumulate, int B, int h, int w,
                              int H, int W, int C, lsn_stream_t stream)
{
    const char *what = "upsample-add backward";
    if (int rc = check_up(what, B, h, w, H, W, C)) return rc;
    if (int rc = check_tensor(what, "grad_out", grad_out, go_pitch, C)) return rc;
    if (int rc = check_tensor(what, "grad_top", grad_top, gt_pitch, C)) return rc;
    const int total = B * h * w * (C / 4);
    if (accumulate)
        hipLaunchKernelGGL(upsample_add_bwd_kernel<true>, pool_grid(total), dim3(POOL_THREADS), 0, stream, grad_out, go_pitch, grad_top,
                           gt_pitch, h, w, H, W, C / 4, total);
    else
        hipLaunchKernelGGL(upsample_add_bwd_kernel<false>, pool_grid(total), dim3(POOL_THREADS), 0, stream, grad_out, go_pitch, grad_top,
                           gt_pitch, h, w, H, W, C / 4, total);
    LSN_HIP(hipGetLastError());
    return 0;
}

int lsn_corner_pool_forward(int mode, const float *x, int x_pitch, float *y, int y_pitch, int accumulate, int B, int H, int W, int C,
                            lsn_stream_t stream)
{
    const char *what = "corner pool forward";
    if (int rc = check_corner(what, mode, B, H, W, C)) return rc;
    if (int rc = check_tensor(what, "x", x, x_pitch, C)) return rc;
    if (int rc = check_tensor(what, "y", y, y_pitch, C)) return rc;
    LSN_CHECK((const float *)y != x, "%s: y must not be x", what);
    const int total = B * (pool_corner_along_x(mode) ? H : W) * (C / 4);
    if (accumulate)
        hipLaunchKernelGGL(corner_pool_fwd_kernel<true>, pool_grid(total), dim3(POOL_THREADS), 0, stream, mode, x, x_pitch, y, y_pitch, B,
                           H, W, C / 4);
    else
        hipLaunchKernelGGL(corner_pool_fwd_kernel<false>, pool_grid(total), dim3(POOL_THREADS), 0, stream, mode, x, x_pitch, y, y_pitch,
                           B, H, W, C / 4);
    LSN_HIP(hipGetLastError());
    return 0;
}

int lsn_corner_pool_backward(int mode, const float *x, int x_pitch, const float *grad_y, int gy_pitch, float *grad_x, int gx_pitch,
                             int accumulate, int B, int H, int W, int C, lsn_stream_t stream)
{
    const char *what = "corner pool backward";
    if (int rc = check_corner(what, mode, B, H, W, C)) return rc;
    if (int rc = check_tensor(what, "x", x, x_pitch, C)) return rc;
    if (int rc = check_tensor(what, "grad_y", grad_y, gy_pitch, C)) return rc;
    if (int rc = check_tensor(what, "grad_x", grad_x, gx_pitch, C)) return rc;
    LSN_CHECK((const float *)grad_x != x && (const float *)grad_x != grad_y, "%s: grad_x must be a buffer of its own", what);
    const int total = B * (pool_corner_along_x(mode) ? H : W) * (C / 4);
    if (accumulate)
        hipLaunchKernelGGL(corner_pool_bwd_kernel<true>, pool_grid(total), dim3(POOL_THREADS), 0, stream, mode, x, x_pitch, grad_y,
                           gy_pitch, grad_x, gx_pitch, B, H, W, C / 4);
    else
        hipLaunchKernelGGL(corner_pool_bwd_kernel<false>, pool_grid(total), dim3(POOL_THREADS), 0, stream, mode, x, x_pitch, grad_y,
                           gy_pitch, grad_x, gx_pitch, B, H, W, C / 4);
    LSN_HIP(hipGetLastError());
    return 0;
}
