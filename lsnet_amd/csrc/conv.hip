// Dense 2-D convolution (groups = 1) on channels-last fp32 tensors as an implicit GEMM on the bf16 matrix pipe with
// split operands (common.h: NP = 6 products of exact 3-way bf16 splits = fp32-equivalent, the default; NP = 3 products
// of 2-way splits; NP = 1 product of the bf16-rounded operands), fp32 accumulation.  Kernels: conv_kernels.h.
//
// The reference runs torch.nn.Conv2d = cuDNN for every dense conv of the path (backbone resnet.py:624-631,
// 261-301; neck fpn.py:171-217; head lsnet_head.py:160-257).
//
//   forward      : out[p][co] = sum_{tap, ci} x[p @ tap][ci] * w[co][tap][ci] (+ bias, ReLU); up to 8 maps per launch
//   backward-data: the same kernel on grad_output with the weights transposed and flipped; a stride-s convolution is
//                  s x s stride-1 convolutions over tap subsets (TapSub), each writing its residue class of input pixels
//   backward-weight: one of three kernels by conv_wgrad_route.h -- the patch kernel of conv_wgrad_kernels.h here, the
//                  fragment-order and the general kernel of the deformable family through dcn.hip's two launchers
//
// Weights reach the kernel in MFMA fragment order (conv_wfrag_kernel), written by lsn_conv2d_prepare_weights -- once per
// optimizer step when the caller keeps the image (the Python mirror caches it per parameter version), or inside the
// one-shot entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "conv_kernels.h"
#include "conv_route.h"
#include "conv_wgrad_kernels.h"
#include "lib_state.h"
#include "prof.h"

namespace lsn {

// bf16 products of these kernels; they have no fp32-MFMA variant: exact mode gets x6.  -1: no kernels (split_dispatch refuses)
static int conv_np() { return math_np() == 0 ? 6 : math_np(); }
static int conv_npl() { return split_npl(conv_np()); }

// ---- deferred weight-gradient reduces (conv_wgrad_kernels.h; include/lsnet_hip.h lsn_wgrad_defer) ----
// While deferral is on for a stream, the partial tiles of its weight-gradient calls (wgrad_part_buffer) come from the stream's
// arena (lib_state.h), which is not reused until the flush, and conv_wgrad_reduce() queues a descriptor instead of launching.
struct RJob {
    bool fold;
    const float *part, *part_b;
    float *gw, *gb;
    size_t n;
    int nb, splits, splits_b, R, Co;
    WgFold f;
};
static int wgrad_flush(Arena *ar);
// (never while the stream is being captured: a queued reduce is host state, a replay would not run it)
static Arena *deferring(hipStream_t st)
{
    Arena *ar = arena_of(st);
    return ar && ar->defer_mb > 0 && !stream_capturing(st) ? ar : nullptr;
}

int wgrad_part_buffer(size_t floats, float **p, hipStream_t st)
{
    if (Arena *ar = deferring(st)) {
        const int rc = arena_alloc(ar, floats, p, wgrad_flush);
        if (rc != 1) return rc;   // 1: the arena could not be allocated, deferral is off now
    }
    return stream_scratch(floats, p, st);
}

static_assert(CR_MAXLV == CV_MAXLV && CR_SK_MAX_TILES == SK_MAX_TILES, "conv_route.h mirrors the library's constants");
static_assert(cr_ncc(1) == cv_ncc(1) && cr_ncc(32) == cv_ncc(32) && cr_ncc(33) == cv_ncc(33), "conv_route.h counts chunks as cv_ncc");

// One launch of a routed tile (conv_route.h): the scratch the route asks for, the LDS attribute, the launch, and the reduce
// launch behind blockIdx.z splits.
template <int TM, int TN, int WM, int WN, int NP, bool UNAL, bool FINE, bool TRANS>
static int launch_conv_tile(ConvArgs &a, hipStream_t st)
{
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const size_t lds = (size_t)2 * SplitCfg<NP>::NPL * BM * 64;
    const int ks = a.ksplit;
    a.sk_part = nullptr, a.sk_cnt = nullptr;
    if (a.sk_n)
        if (int rc = stream_sk_scratch((size_t)2 * a.sk_n * BM * BN, &a.sk_part, &a.sk_cnt, st)) return rc;
    const int rows = ks > 1 ? a.lv[0].P : 0;   // (ks > 1: one level)
    a.part_pix0 = 0, a.part_rows = rows;
    const size_t n = (size_t)rows * a.Co;
    if (ks > 1)
        if (int rc = stream_scratch(n * ks, &a.part, st)) return rc;
    dim3 grid(a.n_dp + a.sk_n, 1, ks);
    auto launch = [&](auto sk) -> int {   // sk: the stream-K form of the kernel
        auto k = conv_mm_kernel<TM, TN, WM, WN, NP, UNAL, FINE, TRANS, decltype(sk)::value>;
        static bool attr_set = false;   // per instantiation
        if (!attr_set) {
            LSN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            attr_set = true;
        }
        hipLaunchKernelGGL(k, grid, dim3(256), lds, st, a);
        return 0;
    };
    if (int rc = a.sk_n ? launch(std::true_type()) : launch(std::false_type())) return rc;
    if (ks > 1) {
        const int blocks = (int)((n / 4 + 255) / 256 < 1024 ? (n / 4 + 255) / 256 : 1024);
        hipLaunchKernelGGL(conv_splitk_reduce_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, st, a.part, a.lv[0].out, a.bias,
                           a.lv[0].res, a.lv[0].gate, (int)n, a.Co, ks, a.relu);
    }
    LSN_HIP(hipGetLastError());
    return 0;
}

enum ConvKind { CONV_FWD, CONV_BWD_DATA, CONV_ROWS };   // CONV_ROWS: conv_mm_rows, its row blocks at 32-bit byte offsets

// The route (conv_route.h) of the launch that `a` describes.
static ConvRoute conv_route_of(const ConvArgs &a, ConvKind kind, bool rows32 = false)
{
    ConvRouteShape s = {};
    s.n = a.nlv;
    for (int i = 0; i < a.nlv; ++i) s.P[i] = a.lv[i].P;
    s.C = a.C, s.xpitch = a.xpitch, s.Co = a.Co, s.taps = a.kh * a.kw;
    s.ostep = a.ostep != 0, s.data_grad = kind == CONV_BWD_DATA, s.rows_gemm = kind == CONV_ROWS, s.rows32 = rows32;
    return conv_route(s);
}

// Writes the route into `a` and runs the tile's kernel; the one place that refuses what the route refuses.
// FINE: the fine MFMA / staging interleave (conv_kernels.h) -- adopted for the two wide tiles after the round-4 sweep; for
// the two narrow ones (Co <= 64) it measured no difference (4216 / 3095 vs 4218 / 3105 us, profiles/r4_conv_tiles.txt)
static int conv_launch(ConvArgs &a, const ConvRoute &r, hipStream_t st)
{
    if (r.unsupported) return fail(LSN_ERR_UNSUPPORTED, "%s", r.unsupported);
    for (int i = 0; i < a.nlv; ++i) a.lv[i].tile0 = r.tile0[i];
    a.ntiles = r.tiles, a.tile_base = 0, a.colblocks = r.colblocks, a.ksplit = r.ks;
    a.n_dp = r.sk.n_dp, a.sk_n = r.sk.sk_n, a.sk_tiles = r.sk.sk_tiles;
    return split_dispatch(conv_np(), [&](auto np) -> int {
        constexpr int NP = decltype(np)::value;
        switch (r.tile) {
        case CT_128x32: return launch_conv_tile<1, 1, 4, 1, NP, false, false, false>(a, st);
        case CT_128x64: return launch_conv_tile<1, 2, 4, 1, NP, false, false, false>(a, st);
        case CT_64x128: return launch_conv_tile<1, 2, 2, 2, NP, false, true, false>(a, st);
        case CT_64x128_UNAL: return launch_conv_tile<1, 2, 2, 2, NP, true, false, false>(a, st);
        case CT_64x256: return launch_conv_tile<2, 2, 1, 4, NP, false, true, false>(a, st);
        case CT_64x256_ROWS: return launch_conv_tile<2, 2, 1, 4, NP, false, true, true>(a, st);
        }
        return fail(LSN_ERR_INVALID, "conv2d: no kernel for tile %d", (int)r.tile);
    });
}

// dcn.hip: out_i[r][0 .. N) = x_i[r][0 .. Cr) . Wt for row blocks i (the backward-data GEMM of the deformable
// convolutions: a 1x1 convolution of grad_output whose N = K * C output columns are the column gradients); wf = the
// fragment image of the (N, 1, Cr) GEMM view.  No profiling span of its own: it runs inside the caller's.
int conv_mm_rows(int n, const float *const *x, float *const *out, const int *rows, int Cr, int xpitch, int N,
                 const unsigned short *wf, hipStream_t st)
{
    LSN_CHECK(n >= 1 && n <= CV_MAXLV && Cr % 4 == 0 && xpitch % 4 == 0 && xpitch >= Cr, "conv_mm_rows: bad arguments");
    ConvArgs a = {};
    a.nlv = n;
    for (int i = 0; i < n; ++i) {
        ConvLvl &L = a.lv[i];
        L.x = x[i], L.out = out[i], L.res = nullptr;
        L.B = 1, L.H = 1, L.W = rows[i], L.Ho = 1, L.Wo = rows[i], L.P = rows[i];
    }
    a.wf = wf;
    a.wf_bytes = (int)cv_wfrag_bytes(N, 1, Cr, conv_npl());
    a.C = Cr, a.Co = N, a.kh = a.kw = 1, a.stride = 1, a.pad_h = a.pad_w = 0, a.dil = 1;
    a.xpitch = xpitch;
    bool rows32 = true;   // the TRANS epilogue stores through a buffer descriptor of each row block: 32-bit byte offsets
    for (int i = 0; i < n; ++i) rows32 = rows32 && (long long)rows[i] * N * 4 < (1ll << 31) - 256;
    return conv_launch(a, conv_route_of(a, CONV_ROWS, rows32), st);
}

// optional folded BatchNorm of a prepare call (all NULL: a plain weight)
struct BnFold {
    const float *gamma = nullptr, *var = nullptr, *beta = nullptr, *mean = nullptr;
    float *shift_out = nullptr;
    float eps = 0.f;
};

static void wfrag_job(WfragJob &j, const float *w, unsigned short *out, int Co, int K, int C, int flipT, const TapSub &ts,
                      const BnFold &bn)
{
    j = WfragJob{};
    j.w = w, j.out = out, j.Co = Co, j.K = K, j.C = C, j.flipT = flipT, j.ts = ts;
    j.bn_gamma = bn.gamma, j.bn_var = bn.var, j.bn_beta = bn.beta, j.bn_mean = bn.mean, j.shift_out = bn.shift_out, j.bn_eps = bn.eps;
}

static int conv_wfrag(const float *w, unsigned short *out, int Co, int K, int C, int flipT, const TapSub &ts, hipStream_t st,
                      const BnFold &bn = BnFold())
{
    WfragJob j;
    wfrag_job(j, w, out, Co, K, C, flipT, ts, bn);
    const long long total = wfrag_threads(j);
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    return split_dispatch(conv_np(), [&](auto np) {
        hipLaunchKernelGGL(conv_wfrag_kernel<SplitCfg<decltype(np)::value>::NPL>, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, st, j);
        return 0;
    });
}

// prof.h span of one launch: 2 P Co C K flops; every operand once (the strided backward-data pass counts grad_out once
// per residue class it launches)
struct ConvProf : ProfSpan {
    static double fl(const ConvArgs &a)
    {
        double px = 0;
        for (int i = 0; i < a.nlv; ++i) px += (double)a.lv[i].P;
        return 2.0 * px * a.Co * a.C * a.kh * a.kw;
    }
    static double by(const ConvArgs &a)
    {
        double e = (double)a.Co * a.C * a.kh * a.kw;
        for (int i = 0; i < a.nlv; ++i)
            e += (double)a.lv[i].B * a.lv[i].H * a.lv[i].W * a.xpitch + (double)a.lv[i].P * a.Co;
        return 4.0 * e;
    }
    ConvProf(int fam, const ConvArgs &a, hipStream_t s) : ProfSpan(fam, fl(a), by(a), s) {}
};

// prof.h launch log: one record per forward / backward-data call (all residue classes of a strided data gradient included)
struct LaunchLog {
    LaunchRec r;
    hipStream_t st;
    bool on;
    LaunchLog(int kind, int n, const lsn_conv_level *lv, int C, int xpitch, int Co, int kh, int kw, int stride, int pad, int dil,
              int relu, hipStream_t s) : st(s), on(launch_log_on())
    {
        if (!on) return;
        memset(&r, 0, sizeof(r));
        int res = 0, gate = 0;
        for (int i = 0; i < n && i < 16; ++i) {
            r.B[i] = lv[i].B, r.H[i] = lv[i].H, r.W[i] = lv[i].W;
            res |= lv[i].residual != nullptr, gate |= lv[i].gate != nullptr;
        }
        const int v[13] = {kind, C, Co, kh, kw, stride, pad, dil, relu, xpitch, n, res, gate};
        memcpy(r.v, v, sizeof(v));
        if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) {
            on = false;
            return;
        }
        (void)hipEventRecord(r.e0, st);
    }
    ~LaunchLog()
    {
        if (!on) return;
        (void)hipEventRecord(r.e1, st);
        launch_log_push(r);
    }
    LaunchLog(const LaunchLog &) = delete;
    LaunchLog &operator=(const LaunchLog &) = delete;
};

static int conv_check(int B, int H, int W, int C, int Co, int kh, int kw, int stride, int pad, int dil, int *Ho,
                      int *Wo)
{
    LSN_CHECK(B > 0 && H > 0 && W > 0 && C > 0 && Co > 0 && kh > 0 && kw > 0, "conv2d: empty tensor");
    LSN_CHECK(stride > 0 && dil > 0 && pad >= 0, "conv2d: bad stride / dilation / padding");
    if (kh * kw > 64) return fail(LSN_ERR_UNSUPPORTED, "conv2d kernel takes at most 64 taps, got %d x %d", kh, kw);
    *Ho = conv_out(H, kh, stride, pad, dil);
    *Wo = conv_out(W, kw, stride, pad, dil);
    LSN_CHECK(*Ho > 0 && *Wo > 0, "conv2d: output size is too small");
    if ((int64_t)B * H * W * C * 4 >= ((int64_t)1 << 31) || (int64_t)Co * kh * kw * C * 4 >= ((int64_t)1 << 31) ||
        (int64_t)B * *Ho * *Wo * Co * 4 >= ((int64_t)1 << 31))
        return fail(LSN_ERR_UNSUPPORTED, "conv2d: tensor too large for 32-bit buffer offsets");
    return 0;
}

// Scratch for a weight image when the caller of a one-shot entry point passes no workspace: stream-ordered allocation.
struct TempImage {
    void *p = nullptr;
    hipStream_t st;
    explicit TempImage(hipStream_t s) : st(s) {}
    int alloc(size_t bytes)
    {
        LSN_HIP(hipMallocAsync(&p, bytes, st));
        lib_stat(STAT_POOL_ALLOCS, 1);
        return 0;
    }
    ~TempImage()
    {
        if (p) (void)hipFreeAsync(p, st);
    }
};

static int conv_forward_impl(int n, const lsn_conv_level *lv, const void *prepared, const float *bias, int C, int xpitch,
                             int Co, int kh, int kw, int stride, int pad, int dil, int relu, hipStream_t st)
{
    LSN_CHECK(n >= 1 && n <= CV_MAXLV && lv && prepared, "conv2d: bad level list");
    LSN_CHECK(xpitch > 0, "conv2d: bad pixel pitch %d", xpitch);
    LaunchLog log(0, n, lv, C, xpitch, Co, kh, kw, stride, pad, dil, relu, st);
    ConvArgs a = {};
    a.nlv = n;
    for (int i = 0; i < n; ++i) {
        ConvLvl &L = a.lv[i];
        LSN_CHECK(lv[i].x && lv[i].out, "conv2d: NULL tensor in level %d", i);
        if (int rc = conv_check(lv[i].B, lv[i].H, lv[i].W, C, Co, kh, kw, stride, pad, dil, &L.Ho, &L.Wo)) return rc;
        if (xpitch != C) {
            // row-merged form: the C "channels" of a tap are C / xpitch horizontally adjacent pixels; they must stay
            // inside the row (the caller pads the image), and the output grid follows the REAL pixels
            LSN_CHECK(kw == 1 && pad == 0 && dil == 1 && C % xpitch == 0, "conv2d: row-merged form needs kw = 1, pad = 0, dil = 1");
            L.Wo = (lv[i].W - C / xpitch) / stride + 1;
            LSN_CHECK(L.Wo > 0, "conv2d: output size is too small");
        }
        L.x = lv[i].x, L.out = lv[i].out, L.B = lv[i].B, L.H = lv[i].H, L.W = lv[i].W;
        L.res = lv[i].residual, L.gate = lv[i].gate;
        L.P = L.B * L.Ho * L.Wo;
    }
    a.bias = bias;
    a.wf = reinterpret_cast<const unsigned short *>(prepared);
    a.wf_bytes = (int)cv_wfrag_bytes(Co, kh * kw, C, conv_npl());
    a.C = C, a.Co = Co, a.kh = kh, a.kw = kw, a.stride = stride, a.pad_h = a.pad_w = pad, a.dil = dil;
    a.xpitch = xpitch;
    a.relu = relu;
    ConvProf prof(PROF_CONV_FWD, a, st);
    return conv_launch(a, conv_route_of(a, CONV_FWD), st);
}

// Residue classes of the transposed convolution (backward-data of a stride-s convolution):
//   grad_in[y, x] = sum over taps (i, j) with (y + pad - i dil) % s == 0 (same for x) of
//                   grad_out[(y + pad - i dil) / s, (x + pad - j dil) / s] . w[:, i, j, :]
// Each class (y % s, x % s) of input pixels is a stride-1 convolution of grad_out with its own subset of the taps (an
// arithmetic progression): no zero-stuffed samples, no wasted products.  Classes without a tap keep the zeros of a memset.
struct BwdClass {
    TapSub ts;
    int py, px, pad_h, pad_w, dstep;
    size_t wf_off;   // byte offset of the class's weight image
};
struct BwdPlan {
    BwdClass cls[64];
    int ncls;
    bool need_zero;
    size_t bytes;
};

static int bwd_plan(int C, int Co, int kh, int kw, int s, int pad, int dil, BwdPlan *pl)
{
    if (s * s > 64) return fail(LSN_ERR_UNSUPPORTED, "conv2d backward-data: stride %d is not supported", s);
    pl->ncls = 0, pl->need_zero = false, pl->bytes = 0;
    auto taps_of = [&](int p, int k, int &t0, int &tstep, int &nt) {
        t0 = -1, tstep = 1, nt = 0;
        int prev = -1;
        for (int t = 0; t < k; ++t)
            if (((p + pad - t * dil) % s + s) % s == 0) {
                if (nt == 0) t0 = t;
                if (nt == 1) tstep = t - prev;
                prev = t;
                ++nt;
            }
    };
    for (int py = 0; py < s; ++py)
        for (int px = 0; px < s; ++px) {
            BwdClass c;
            c.py = py, c.px = px;
            taps_of(py, kh, c.ts.i0, c.ts.istep, c.ts.ni);
            taps_of(px, kw, c.ts.j0, c.ts.jstep, c.ts.nj);
            c.ts.kw = kw;
            if (c.ts.ni == 0 || c.ts.nj == 0) {
                pl->need_zero = true;
                continue;
            }
            // y_in = yy + q0 - m d' (m-th tap of the subset), d' = istep dil / s; as a correlation over the reversed
            // subset: y_in = yy - P + m' d' with P = (ni - 1) d' - q0
            const int dstep_h = c.ts.istep * dil / s, dstep_w = c.ts.jstep * dil / s;
            if (c.ts.ni > 1 && c.ts.nj > 1 && dstep_h != dstep_w)
                return fail(LSN_ERR_UNSUPPORTED, "conv2d backward-data: unequal tap spacing");
            c.dstep = c.ts.ni > 1 ? dstep_h : (c.ts.nj > 1 ? dstep_w : 1);
            if ((c.ts.ni > 1 && c.ts.istep * dil % s != 0) || (c.ts.nj > 1 && c.ts.jstep * dil % s != 0))
                return fail(LSN_ERR_UNSUPPORTED, "conv2d backward-data: stride / dilation combination");
            const int q0h = (py + pad - c.ts.i0 * dil) / s, q0w = (px + pad - c.ts.j0 * dil) / s;
            c.pad_h = (c.ts.ni - 1) * c.dstep - q0h;
            c.pad_w = (c.ts.nj - 1) * c.dstep - q0w;
            c.wf_off = pl->bytes;
            // the transposed convolution reduces over the forward Co and produces the forward C
            pl->bytes += cv_wfrag_bytes(C, c.ts.ni * c.ts.nj, Co, conv_npl());
            pl->cls[pl->ncls++] = c;
        }
    return 0;
}

// grad_in of every level (B, H, W, C) from grad_out (B, Ho, Wo, Co): lv[i].x = grad_out, lv[i].out = grad_in, and
// lv[i].B / H / W are the INPUT sizes of the forward convolution
static int conv_backward_data_impl(int n, const lsn_conv_level *lv, const void *prepared, int C, int Co, int kh, int kw,
                                   int stride, int pad, int dil, hipStream_t st)
{
    LSN_CHECK(n >= 1 && n <= CV_MAXLV && lv && prepared, "conv2d backward: bad arguments");
    LaunchLog log(1, n, lv, C, C, Co, kh, kw, stride, pad, dil, 0, st);
    const int s = stride;
    int Ho[CV_MAXLV], Wo[CV_MAXLV];
    for (int i = 0; i < n; ++i) {
        LSN_CHECK(lv[i].x && lv[i].out, "conv2d backward: NULL tensor in level %d", i);
        if (int rc = conv_check(lv[i].B, lv[i].H, lv[i].W, C, Co, kh, kw, stride, pad, dil, &Ho[i], &Wo[i])) return rc;
    }
    if (s > 1 && n > 1) return fail(LSN_ERR_UNSUPPORTED, "conv2d backward-data: strided convolutions take one level per call");
    BwdPlan pl;
    if (int rc = bwd_plan(C, Co, kh, kw, s, pad, dil, &pl)) return rc;
    const int H = lv[0].H, W = lv[0].W, B = lv[0].B;
    bool epi = false;   // a residual (another path's gradient of the same tensor) / ReLU gate in the epilogue
    for (int i = 0; i < n; ++i) epi = epi || lv[i].residual || lv[i].gate;
    if (epi && pl.need_zero)
        return fail(LSN_ERR_UNSUPPORTED, "conv2d backward-data: residual / gate with residue classes that have no tap");
    if (epi && C % 4 != 0) return fail(LSN_ERR_UNSUPPORTED, "conv2d backward-data: residual / gate need C %% 4 == 0");
    if (pl.need_zero) LSN_HIP(hipMemsetAsync(lv[0].out, 0, sizeof(float) * (size_t)B * H * W * C, st));
    for (int ci = 0; ci < pl.ncls; ++ci) {
        const BwdClass &c = pl.cls[ci];
        const int Hc = c.py < H ? (H - c.py + s - 1) / s : 0, Wc = c.px < W ? (W - c.px + s - 1) / s : 0;
        if (s > 1 && (Hc == 0 || Wc == 0)) continue;
        ConvArgs a = {};
        a.wf = reinterpret_cast<const unsigned short *>(reinterpret_cast<const unsigned char *>(prepared) + c.wf_off);
        a.wf_bytes = (int)cv_wfrag_bytes(C, c.ts.ni * c.ts.nj, Co, conv_npl());
        a.nlv = n;
        for (int i = 0; i < n; ++i) {
            ConvLvl &L = a.lv[i];
            L.x = lv[i].x, L.out = lv[i].out, L.res = lv[i].residual, L.gate = lv[i].gate;
            L.B = lv[i].B, L.H = Ho[i], L.W = Wo[i];
            L.Ho = s > 1 ? Hc : lv[i].H, L.Wo = s > 1 ? Wc : lv[i].W;
            L.P = L.B * L.Ho * L.Wo;
        }
        a.C = Co, a.Co = C, a.kh = c.ts.ni, a.kw = c.ts.nj, a.stride = 1;
        a.xpitch = Co;
        a.pad_h = c.pad_h, a.pad_w = c.pad_w, a.dil = c.dstep;
        if (s > 1) a.ostep = s, a.oy0 = c.py, a.ox0 = c.px, a.OH = H, a.OW = W;
        ConvProf prof(PROF_CONV_BWD_DATA, a, st);
        if (int rc = conv_launch(a, conv_route_of(a, CONV_BWD_DATA), st)) return rc;
    }
    return 0;
}

static int64_t prepared_bytes(int kind, int C, int Co, int kh, int kw, int stride, int pad, int dil)
{
    if (kind == 0) return (int64_t)cv_wfrag_bytes(Co, kh * kw, C, conv_npl());
    if (kind == 2) return (int64_t)cv_wfrag_bytes(kh * kw * C, 1, Co, conv_npl());   // deformable backward GEMM: N = K C columns
    BwdPlan pl;
    if (bwd_plan(C, Co, kh, kw, stride, pad, dil, &pl)) return -1;
    return (int64_t)pl.bytes;
}

static int bn_fold_of(const lsn_conv_wprep &p, BnFold *bn)
{
    *bn = BnFold();
    if (!p.bn_gamma) return 0;
    LSN_CHECK(p.bn_var, "conv2d prepare: incomplete BatchNorm description");
    if (p.kind == 0)
        LSN_CHECK(p.bn_beta && p.bn_mean && p.shift_out, "conv2d prepare: incomplete BatchNorm description");
    else
        LSN_CHECK(!p.shift_out, "conv2d prepare: the shift belongs to the forward image");
    bn->gamma = p.bn_gamma, bn->var = p.bn_var, bn->beta = p.bn_beta, bn->mean = p.bn_mean, bn->shift_out = p.shift_out;
    bn->eps = p.bn_eps;
    return 0;
}

static int prepare_weights(int kind, const float *w, void *prepared, int C, int Co, int kh, int kw, int stride, int pad,
                           int dil, hipStream_t st, const BnFold &bn = BnFold())
{
    LSN_CHECK(w && prepared, "conv2d prepare: NULL pointer");
    LSN_CHECK(C > 0 && Co > 0 && kh > 0 && kw > 0, "conv2d prepare: bad weight shape");
    // (a valid convolution that this build does not serve -- the answer of conv_check, which the one-shot entries reach only
    // behind this call)
    if (kh * kw > 64) return fail(LSN_ERR_UNSUPPORTED, "conv2d kernel takes at most 64 taps, got %d x %d", kh, kw);
    if (prepared_bytes(kind, C, Co, kh, kw, stride, pad, dil) >= ((int64_t)1 << 31))
        return fail(LSN_ERR_UNSUPPORTED, "conv2d: weight too large for 32-bit buffer offsets");
    if (kind == 0) {
        if (int rc = conv_wfrag(w, reinterpret_cast<unsigned short *>(prepared), Co, kh * kw, C, 0, TapSub{}, st, bn)) return rc;
    } else if (kind == 2) {
        if (int rc = conv_wfrag(w, reinterpret_cast<unsigned short *>(prepared), kh * kw * C, 1, Co, 1, TapSub{0, 1, 1, 0, 1, 1, 1}, st,
                                bn))
            return rc;
    } else {
        BwdPlan pl;
        if (int rc = bwd_plan(C, Co, kh, kw, stride, pad, dil, &pl)) return rc;
        for (int ci = 0; ci < pl.ncls; ++ci)
            if (int rc = conv_wfrag(w, reinterpret_cast<unsigned short *>(reinterpret_cast<unsigned char *>(prepared) + pl.cls[ci].wf_off),
                                    C, kh * kw, Co, 1, pl.cls[ci].ts, st, bn))
                return rc;
    }
    LSN_HIP(hipGetLastError());
    return 0;
}

// ---- weight / bias gradient (conv_wgrad_kernels.h) ----
static_assert(CW_MAXLV <= CV_MAXLV, "WgArgs holds every level of a validated call");
static int fold_jobs(const WgFoldJobs *fold) { return fold ? fold->njobs : 1; }

// UN_OK: the configuration also serves Co % 4 != 0 (conv_wgrad_route.h sends no other one such a call)
template <int TI, int TJ, int TG, int WI, int WJ, int PMAX, bool UN_OK>
static int launch_wgrad_cfg(WgArgs &a, const ConvWgradCall &c, hipStream_t st)
{
    float *const gw = c.gw, *const gb = c.gb;
    const bool un = a.Co % 4 != 0;
    LSN_CHECK(UN_OK || !un, "conv2d backward-weight: Co = %d on an aligned configuration of the patch kernel", a.Co);
    constexpr int BN = WI * TI * 32, BM = WJ * TJ * 32;
    const int npl = conv_npl(), K = a.kh * a.kw;
    const int blocks = cdiv(a.Co, BM) * cdiv(a.C, BN);
    const size_t nW = (size_t)a.Co * K * a.C;
    const int nj = fold_jobs(c.fold);   // > 1: the levels are jobs with their own outputs; every split stays inside one level
    int S = 512 / (blocks * nj);   // one round of workgroups (rounds 3 / 4 rounded to nearest: 516 .. 540 on 512 slots)
    const size_t cap = ((size_t)192 << 20) / 4 / (nW + a.Co) / nj;   // partial tiles: at most 192 MB
    if ((size_t)S > cap) S = (int)cap;
    if (S > a.nseg / nj / 6) S = a.nseg / nj / 6;   // a split should run long enough to amortise its prologue and its partial tile
    if (S < 1) S = 1;
    S *= nj;
    float *part = nullptr;
    if (int rc = wgrad_part_buffer((size_t)S * (nW + a.Co) + 16, &part, st)) return rc;
    a.part = part;
    a.part_b = part + (((size_t)S * nW + 3) & ~(size_t)3);
    a.want_bias = gb != nullptr;
    constexpr int XP = 1024 / BN, GP = 1024 / BM;   // pixels per staging pass (conv_wgrad_kernel)
    constexpr size_t lds_plane = (size_t)2 * ((PMAX + XP - 1) / XP * XP * BN * 2 + (16 + GP - 1) / GP * GP * BM * 2);
    static_assert(lds_plane <= 32 * 1024, "three planes per operand stay below the 160 KB of a workgroup");
    const size_t lds = lds_plane * npl;
    dim3 grid(blocks, S);
    LSN_CHECK((long long)a.nseg * (S + 1) < (1ll << 32), "conv2d backward-weight: %d segments x %d splits exceed the kernel's 32-bit split arithmetic", a.nseg, S);
    auto launch = [&](auto kern) -> int {
        LSN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, a);
        return 0;
    };
    int rc;
    // the fine MFMA / staging interleave (conv_wgrad_kernels.h FINE; round-4 A/B over the step's layer shapes 3.57 -> 3.41 ms)
    // wherever it compiles without spills: not the unaligned form, not the 4 x 1 wave layout of the narrow 3x3 form
    constexpr bool FINE = !(TG == 9 && WI == 4);
    rc = split_dispatch(conv_np(), [&](auto np) {
        constexpr int NP = decltype(np)::value;
        if constexpr (NP == 1 && TG == 9 && WI == 4) {   // (not instantiated: see cw_patch_ok)
            return fail(LSN_ERR_INVALID, "conv2d backward-weight: no one-product form of the narrow 3x3 kernel");
        } else {
            if constexpr (UN_OK) {
                if (un) return launch(conv_wgrad_kernel<TI, TJ, TG, WI, WJ, NP, true, PMAX, false>);
            }
            return launch(conv_wgrad_kernel<TI, TJ, TG, WI, WJ, NP, false, PMAX, FINE>);
        }
    });
    if (rc) return rc;
    return conv_wgrad_reduce(a.part, gw, nW, a.part_b, gb, a.Co, S, S, c.accumulate, c.fold, st);
}

// Lanes that share a float4 of the reduce: each sums PER_LANE partial tiles on its own before the xor-shuffles (>= PER_LANE / 2
// loads per lane; a wave's lanes share 64 / LS elements).  Round-4 sweep (tools/ubench/wgrad_ab rule / bn, us per step of the layer
// mix): 4: 3374 / 2945, 8: 3284 / 2729, 16: 3254 / 2650, 32: 3252 / 2642 -- fewer, longer lanes win until the loads in flight run out.
static int reduce_ls(int splits)
{
    constexpr int PER_LANE = 16;
    int LS = 1;
    while (LS < 64 && LS * PER_LANE <= splits) LS <<= 1;
    return LS;
}

// lib_state.h.  With a fold, gb is the entry point's dummy bias gradient (it only makes the main kernels write the per-channel
// sums of g) and conv_wgrad_reduce_bn_kernel is the only writer of grad_w / grad_gamma / grad_beta.
int conv_wgrad_reduce(const float *part, float *gw, size_t n, const float *part_b, float *gb, int nb, int splits, int splits_b,
                      int accumulate, const WgFoldJobs *fold, hipStream_t st)
{
    const int nj = fold_jobs(fold);   // (splits / splits_b count ALL jobs' partial tiles)
    if (fold)
        LSN_CHECK(part_b && nb > 0 && n % ((size_t)nb * 4) == 0 && splits % nj == 0 && splits_b % nj == 0,
                  "conv2d backward-weight (folded norm): bad partial layout");
    if (Arena *ar = accumulate ? deferring(st) : nullptr) {
        // queue instead of launching.  A gradient that already has a queued job is reduced first: two jobs of one launch must
        // not add onto the same addresses.
        bool clash = false;
        for (const RJob &q : *ar->jobs)
            for (int j = 0; j < nj; ++j) {
                const float *tw = fold ? (nj > 1 ? fold->gw[j] : gw) : gw;
                clash = clash || q.gw == tw || (gb && q.gb == gb) || (fold && q.fold && q.f.dgamma == fold->f[j].dgamma);
            }
        if (clash)
            if (int rc = wgrad_flush(ar)) return rc;   // (the arena is NOT rewound here: this call's partial tiles are in it)
        for (int j = 0; j < nj; ++j) {   // (plain: one job, the caller's own pointers)
            RJob q = {};
            q.fold = fold != nullptr;
            q.part = part + (size_t)j * (splits / nj) * n, q.part_b = q.fold ? part_b + (size_t)j * (splits_b / nj) * nb : part_b;
            q.gw = nj > 1 ? fold->gw[j] : gw, q.gb = q.fold ? nullptr : gb;
            q.n = n, q.nb = nb, q.splits = splits / nj, q.splits_b = splits_b / nj;
            if (q.fold) q.R = (int)(n / nb), q.Co = nb, q.f = fold->f[j];
            ar->jobs->push_back(q);
        }
        if ((long long)(ar->used * sizeof(float)) > (ar->defer_mb << 20)) {
            if (int rc = wgrad_flush(ar)) return rc;
            ar->used = 0;   // every queued tile has been consumed (in stream order): the arena starts over
        }
        return 0;
    }
    const int LS = reduce_ls(splits / nj);
    if (fold) {
        hipLaunchKernelGGL(conv_wgrad_reduce_bn_kernel, dim3(nb, nj), dim3(256), 0, st, part, gw, (int)(n / nb), nb, part_b,
                           splits / nj, splits_b / nj, accumulate, LS, *fold);
        LSN_HIP(hipGetLastError());
        return 0;
    }
    const size_t thr = n / 4 * LS;
    const int rb = (int)((thr + 255) / 256 < 4096 ? (thr + 255) / 256 : 4096);
    hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3(rb > 0 ? rb : 1), dim3(256), 0, st, part, gw, n, part_b, gb, nb, splits,
                       splits_b, accumulate, LS);
    LSN_HIP(hipGetLastError());
    return 0;
}

static int wgrad_flush(Arena *ar)
{
    std::vector<RJob> &jobs = *ar->jobs;
    if (jobs.empty()) return 0;
    hipStream_t st = ar->st;
    double bytes = 0;
    for (const RJob &q : jobs) bytes += 4.0 * ((double)q.splits * q.n + 2.0 * q.n);
    ProfSpan prof(PROF_CONV_WGRAD, 0.0, bytes, st);   // (the family's time includes its reduces, wherever they are launched)
    RJobsPlain P = {};
    RJobsFold F = {};
    int pblk = 0, fblk = 0;
    auto launch_plain = [&]() {
        if (P.njobs) hipLaunchKernelGGL(conv_wgrad_reduce_multi_kernel, dim3(pblk), dim3(256), 0, st, P);
        P.njobs = 0, pblk = 0;
    };
    auto launch_fold = [&]() {
        if (F.njobs) hipLaunchKernelGGL(conv_wgrad_reduce_bn_multi_kernel, dim3(fblk), dim3(256), 0, st, F);
        F.njobs = 0, fblk = 0;
    };
    for (const RJob &q : jobs) {
        const int LS = reduce_ls(q.splits);
        if (q.fold) {
            if (F.njobs == RJ_MAX) launch_fold();
            RJobFold &d = F.j[F.njobs++];
            d.part = q.part, d.part_b = q.part_b, d.gw = q.gw, d.f = q.f, d.R = q.R, d.Co = q.Co, d.splits = q.splits,
            d.splits_b = q.splits_b, d.LS = LS, d.blk0 = fblk;
            fblk += q.Co;
        } else {
            if (P.njobs == RJ_MAX) launch_plain();
            const size_t thr = q.n / 4 * LS;
            const int rb = (int)((thr + 255) / 256 < 4096 ? (thr + 255) / 256 : 4096);
            RJobPlain &d = P.j[P.njobs++];
            d.part = q.part, d.part_b = q.part_b, d.gw = q.gw, d.gb = q.gb, d.n = q.n, d.nb = q.nb, d.splits = q.splits,
            d.splits_b = q.splits_b, d.LS = LS, d.blk0 = pblk, d.nblk = rb > 0 ? rb : 1;
            pblk += d.nblk;
        }
    }
    launch_plain();
    launch_fold();
    jobs.clear();
    LSN_HIP(hipGetLastError());
    return 0;
}

// The patch kernel on a call that conv_wgrad_route.h sent here (CW_PATCH, or CW_PATCH_JOBS with the jobs as levels)
static int conv_wgrad_patch(const ConvWgradCall &c, hipStream_t st)
{
    const ConvWgradShape &s = c.s;
    LSN_CHECK(cw_patch_ok(s), "conv2d backward-weight: not a shape of the patch kernel");
    WgArgs a = {};
    int seg = 0;
    for (int i = 0; i < s.n; ++i) {
        WgLvl &L = a.lv[i];
        L.x = c.x[i], L.go = c.go[i], L.B = s.lv[i].B, L.H = s.lv[i].H, L.W = s.lv[i].W, L.Ho = s.lv[i].Ho, L.Wo = s.lv[i].Wo;
        L.nsx = cdiv(L.Wo, 16);
        L.seg0 = seg;
        seg += L.B * L.Ho * L.nsx;
    }
    a.nlv = s.n, a.nseg = seg;
    a.C = s.C, a.Co = s.Co, a.kh = s.kh, a.kw = s.kw, a.stride = s.stride, a.pad = c.pad, a.dil = s.dil;
    a.cstep = s.kw == 1 ? s.stride : 1;
    a.PW = s.kw == 1 ? 16 : 15 * s.stride + (s.kw - 1) * s.dil + 1;
    static_assert(3 * (15 + 2 + 1) == 54 && 1 * 16 == 16, "the patches of the two geometries are the PMAX of their configurations");
    if (s.kh * s.kw == 1) {   // one tap: 32 .. 64 channels per wave on either side, by the layer's width
        // (round-4 sweep, profiles/r4_wgrad_tiles.txt: forcing any one of the four tiles on every layer loses to this
        // width rule by 0 .. 25 %)
        if (s.C <= 64)
            return s.Co <= 64 ? launch_wgrad_cfg<1, 1, 1, 2, 2, 16, false>(a, c, st) : launch_wgrad_cfg<1, 2, 1, 2, 2, 16, false>(a, c, st);
        return s.Co <= 64 ? launch_wgrad_cfg<2, 1, 1, 2, 2, 16, false>(a, c, st) : launch_wgrad_cfg<2, 2, 1, 2, 2, 16, false>(a, c, st);
    }
    if (s.Co <= 32) return launch_wgrad_cfg<1, 1, 9, 4, 1, 54, true>(a, c, st);
    return launch_wgrad_cfg<1, 1, 9, 2, 2, 54, false>(a, c, st);
}

// The one description of a weight-gradient call: arguments checked, output sizes and pixel counts filled in, and what the
// route depends on beside the shape (pointer alignment, math mode, debug word) read here, once.
static int conv_wgrad_call(ConvWgradCall &c, int n, const lsn_conv_level *lv, float *gw, float *gb, int C, int Co, int kh, int kw,
                           int stride, int pad, int dil, int accumulate, const WgFoldJobs *fold)
{
    if (fold && ((size_t)kh * kw * C) % 4 != 0)
        return fail(LSN_ERR_UNSUPPORTED, "conv2d backward-weight (folded norm): kh * kw * C %% 4 != 0");
    LSN_CHECK(C > 0 && Co > 0 && kh > 0 && kw > 0 && stride > 0 && dil > 0 && pad >= 0, "conv2d backward-weight: bad shape");
    LSN_CHECK(n >= 1 && n <= CW_MAXLV && lv && gw, "conv2d backward-weight: bad arguments");
    ConvWgradShape &s = c.s;
    s.aligned16 = true;
    for (int i = 0; i < n; ++i) {
        ConvWgradLevel &L = s.lv[i];
        L.B = lv[i].B, L.H = lv[i].H, L.W = lv[i].W;
        LSN_CHECK(lv[i].x && lv[i].grad_out && L.B > 0 && L.H > 0 && L.W > 0, "conv2d backward-weight: bad level %d", i);
        L.Ho = conv_out(L.H, kh, stride, pad, dil), L.Wo = conv_out(L.W, kw, stride, pad, dil);
        LSN_CHECK(L.Ho > 0 && L.Wo > 0, "conv2d backward-weight: output size is too small");
        if ((int64_t)L.B * L.H * L.W * C >= ((int64_t)1 << 31) || (int64_t)L.B * L.Ho * L.Wo * Co >= ((int64_t)1 << 31))
            return fail(LSN_ERR_UNSUPPORTED, "conv2d backward-weight: tensor too large for 32-bit indexing");
        L.P = L.B * L.Ho * L.Wo;
        c.x[i] = lv[i].x, c.go[i] = lv[i].grad_out;
        s.aligned16 = s.aligned16 && ((reinterpret_cast<uintptr_t>(c.x[i]) | reinterpret_cast<uintptr_t>(c.go[i])) & 15) == 0;
    }
    s.n = n, s.C = C, s.Co = Co, s.kh = kh, s.kw = kw, s.stride = stride, s.dil = dil;
    s.np = math_np(), s.npl = split_npl(s.np), s.general_gemms = general_gemms_only(), s.fold_jobs = fold ? fold->njobs : 0;
    c.pad = pad, c.accumulate = accumulate ? 1 : 0, c.gw = gw, c.gb = gb, c.fold = fold;
    return 0;
}

// Weight gradient of a dense convolution, summed over the levels (input maps that share the weight): validate, route, launch.
// With a fold the levels are its jobs, gw / gb job 0's grad_w / grad_beta: grad_beta stands in as the bias gradient, so that the
// main kernels write the per-channel partial sums of g, and the fold-aware reduce is the only writer of the three outputs.
static int conv_wgrad(int n, const lsn_conv_level *lv, float *gw, float *gb, int C, int Co, int kh, int kw, int stride, int pad,
                      int dil, int accumulate, const WgFoldJobs *fold, hipStream_t st)
{
    ConvWgradCall c;
    if (int rc = conv_wgrad_call(c, n, lv, gw, gb, C, Co, kh, kw, stride, pad, dil, accumulate, fold)) return rc;
    const ConvWgradShape &s = c.s;
    const ConvWgradRoute route = conv_wgrad_route(s);
    if (s.fold_jobs > 1 && route != CW_PATCH_JOBS) {   // no shared launch: every job as a call of its own
        for (int j = 0; j < n; ++j) {
            WgFoldJobs one = {};
            one.f[0] = fold->f[j], one.gw[0] = fold->gw[j], one.njobs = 1;
            if (int rc = conv_wgrad(1, &lv[j], one.gw[0], one.f[0].dbeta, C, Co, kh, kw, stride, pad, dil, accumulate, &one, st)) return rc;
        }
        return 0;
    }
    // the family's account: 2 px Co C K flops, every operand once
    double px = 0, in_el = 0;
    for (int i = 0; i < s.n; ++i) px += (double)s.lv[i].P, in_el += (double)s.lv[i].B * s.lv[i].H * s.lv[i].W * s.C;
    const double K = (double)s.kh * s.kw;
    ProfSpan prof(PROF_CONV_WGRAD, 2.0 * px * s.Co * s.C * K, 4.0 * (in_el + px * s.Co + s.Co * K * s.C), st);
    switch (route) {
    case CW_DENSE_MM: return conv_wgrad_dense_mm(c, st);
    case CW_PATCH:
    case CW_PATCH_JOBS: return conv_wgrad_patch(c, st);
    default: return conv_wgrad_general(c, st);
    }
}

// ---- every stale image of a step in one launch ----
static WfragJob *g_jobs_dev = nullptr;
static size_t g_jobs_cap = 0;
static std::vector<WfragJob> g_jobs_host;   // what the device table holds

static int prepare_weights_multi(int n, const lsn_conv_wprep *it, hipStream_t st)
{
    LSN_CHECK(n >= 0 && (n == 0 || it), "conv2d prepare: bad item list");
    std::vector<WfragJob> jobs;
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        const lsn_conv_wprep &p = it[i];
        LSN_CHECK(p.w && p.prepared && p.C > 0 && p.Co > 0 && p.kh > 0 && p.kw > 0 && p.kh * p.kw <= 64,
                  "conv2d prepare: bad item %d", i);
        if (prepared_bytes(p.kind, p.C, p.Co, p.kh, p.kw, p.stride, p.pad, p.dil) >= ((int64_t)1 << 31))
            return fail(LSN_ERR_UNSUPPORTED, "conv2d: weight too large for 32-bit buffer offsets");
        BnFold bn;
        if (int rc = bn_fold_of(p, &bn)) return rc;
        auto add = [&](void *out, int Co, int K, int C, int flipT, const TapSub &ts) {
            WfragJob j;
            wfrag_job(j, p.w, reinterpret_cast<unsigned short *>(out), Co, K, C, flipT, ts, bn);
            j.start = total;
            total += wfrag_threads(j);
            jobs.push_back(j);
        };
        if (p.kind == 0) {
            add(p.prepared, p.Co, p.kh * p.kw, p.C, 0, TapSub{});
        } else if (p.kind == 2) {
            add(p.prepared, p.kh * p.kw * p.C, 1, p.Co, 1, TapSub{0, 1, 1, 0, 1, 1, 1});
        } else {
            BwdPlan pl;
            if (int rc = bwd_plan(p.C, p.Co, p.kh, p.kw, p.stride, p.pad, p.dil, &pl)) return rc;
            for (int c = 0; c < pl.ncls; ++c)
                add(reinterpret_cast<unsigned char *>(p.prepared) + pl.cls[c].wf_off, p.C, p.kh * p.kw, p.Co, 1, pl.cls[c].ts);
        }
    }
    if (jobs.empty()) return 0;
    const size_t bytes = jobs.size() * sizeof(WfragJob);
    const bool same = jobs.size() == g_jobs_host.size() && memcmp(jobs.data(), g_jobs_host.data(), bytes) == 0;
    if (!same) {   // the table changes only when the set of weights does (first steps): upload then, reuse afterwards
        if (jobs.size() > g_jobs_cap) {
            // (an outgrown table is retired, not freed: a captured graph may hold its address)
            LSN_HIP(hipMalloc(reinterpret_cast<void **>(&g_jobs_dev), (jobs.size() + 64) * sizeof(WfragJob)));
            lib_stat(STAT_MALLOCS, 1), lib_stat(STAT_HELD_BYTES, (long long)((jobs.size() + 64) * sizeof(WfragJob)));
            g_jobs_cap = jobs.size() + 64;
        }
        LSN_HIP(hipStreamSynchronize(st));   // (an earlier launch may still read the old table)
        lib_stat(STAT_BLOCKING_SYNCS, 1);
        LSN_HIP(hipMemcpy(g_jobs_dev, jobs.data(), bytes, hipMemcpyHostToDevice));
        g_jobs_host = jobs;
    }
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    if (int rc = split_dispatch(conv_np(), [&](auto np) {
            hipLaunchKernelGGL(conv_wfrag_multi_kernel<SplitCfg<decltype(np)::value>::NPL>, dim3(blocks), dim3(256), 0, st, g_jobs_dev,
                               (int)jobs.size(), total);
            return 0;
        }))
        return rc;
    LSN_HIP(hipGetLastError());
    return 0;
}

}  // namespace lsn

extern "C" {

int lsn_wgrad_defer(int max_mbytes, lsn_stream_t stream)
{
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    lsn::Arena *ar = lsn::arena_of(st);
    if (max_mbytes > 0) {
        if (int rc = lsn::arena_get(st, &ar)) return rc;
        if (!ar->jobs) ar->jobs = new std::vector<lsn::RJob>();
        ar->jobs->clear();   // (a step that died half-way may have left descriptors behind: they are dropped, not run)
        ar->used = 0;
        ar->defer_mb = max_mbytes;
        return 0;
    }
    if (!ar) return 0;
    const int rc = lsn::wgrad_flush(ar);
    ar->defer_mb = 0, ar->used = 0;
    return rc;
}

int lsn_wgrad_flush(lsn_stream_t stream)
{
    lsn::Arena *ar = lsn::arena_of(reinterpret_cast<hipStream_t>(stream));
    if (!ar) return 0;
    const int rc = lsn::wgrad_flush(ar);
    ar->used = 0;
    return rc;
}

int lsn_conv2d_backward_weight_multi(int n_levels, const lsn_conv_level *levels, float *grad_w, float *grad_bias, int C,
                                     int Co, int kh, int kw, int stride, int pad, int dil, int accumulate,
                                     lsn_stream_t stream)
{
    return lsn::conv_wgrad(n_levels, levels, grad_w, grad_bias, C, Co, kh, kw, stride, pad, dil, accumulate, nullptr,
                           reinterpret_cast<hipStream_t>(stream));
}

int lsn_conv2d_backward_weight(const float *x, const float *grad_out, float *grad_w, float *grad_bias, int B, int H,
                               int W, int C, int Co, int kh, int kw, int stride, int pad, int dil, int accumulate,
                               lsn_stream_t stream)
{
    lsn_conv_level L = {};
    L.x = x, L.grad_out = grad_out, L.B = B, L.H = H, L.W = W;
    return lsn_conv2d_backward_weight_multi(1, &L, grad_w, grad_bias, C, Co, kh, kw, stride, pad, dil, accumulate, stream);
}

int lsn_conv2d_backward_weight_bn(const float *x, const float *g, const float *w, const float *bn_gamma, const float *bn_mean,
                                  const float *bn_var, float bn_eps, float *grad_w, float *grad_gamma, float *grad_beta, int B,
                                  int H, int W, int C, int Co, int kh, int kw, int stride, int pad, int dil, int accumulate,
                                  lsn_stream_t stream)
{
    LSN_CHECK(x && g && w && bn_gamma && bn_mean && bn_var && grad_w && grad_gamma && grad_beta,
              "conv2d backward-weight (folded norm): NULL pointer");
    const lsn_wgrad_bn_job q = {x, g, w, bn_gamma, bn_mean, bn_var, bn_eps, grad_w, grad_gamma, grad_beta};
    return lsn_conv2d_backward_weight_bn_jobs(1, &q, B, H, W, C, Co, kh, kw, stride, pad, dil, accumulate, stream);
}

int lsn_conv2d_backward_weight_bn_jobs(int n_jobs, const lsn_wgrad_bn_job *jobs, int B, int H, int W, int C, int Co, int kh, int kw,
                                       int stride, int pad, int dil, int accumulate, lsn_stream_t stream)
{
    LSN_CHECK(n_jobs >= 1 && n_jobs <= 8 && jobs, "conv2d backward-weight jobs: 1 .. 8 jobs");
    lsn::WgFoldJobs f = {};
    lsn_conv_level lv[8] = {};
    for (int j = 0; j < n_jobs; ++j) {
        const lsn_wgrad_bn_job &q = jobs[j];
        LSN_CHECK(q.x && q.g && q.w && q.bn_gamma && q.bn_mean && q.bn_var && q.grad_w && q.grad_gamma && q.grad_beta,
                  "conv2d backward-weight jobs: NULL pointer in job %d", j);
        f.f[j] = lsn::WgFold{q.w, q.bn_gamma, q.bn_mean, q.bn_var, q.grad_gamma, q.grad_beta, q.bn_eps};
        f.gw[j] = q.grad_w;
        lv[j].x = q.x, lv[j].grad_out = q.g, lv[j].B = B, lv[j].H = H, lv[j].W = W;
    }
    f.njobs = n_jobs;
    return lsn::conv_wgrad(n_jobs, lv, f.gw[0], f.f[0].dbeta, C, Co, kh, kw, stride, pad, dil, accumulate, &f,
                           reinterpret_cast<hipStream_t>(stream));
}

int lsn_conv2d_prepare_weights_multi(int n_items, const lsn_conv_wprep *items, lsn_stream_t stream)
{
    return lsn::prepare_weights_multi(n_items, items, reinterpret_cast<hipStream_t>(stream));
}

int64_t lsn_conv2d_prepared_bytes(int kind, int C, int Co, int kh, int kw, int stride, int pad, int dil)
{
    return lsn::prepared_bytes(kind, C, Co, kh, kw, stride, pad, dil);
}

int lsn_conv2d_prepare_weights(int kind, const float *w, void *prepared, int C, int Co, int kh, int kw, int stride,
                               int pad, int dil, lsn_stream_t stream)
{
    return lsn::prepare_weights(kind, w, prepared, C, Co, kh, kw, stride, pad, dil, reinterpret_cast<hipStream_t>(stream));
}

int lsn_conv2d_prepare_weights_item(const lsn_conv_wprep *item, lsn_stream_t stream)
{
    LSN_CHECK(item != nullptr, "conv2d prepare: NULL item");
    lsn::BnFold bn;
    if (int rc = lsn::bn_fold_of(*item, &bn)) return rc;
    return lsn::prepare_weights(item->kind, item->w, item->prepared, item->C, item->Co, item->kh, item->kw, item->stride,
                                item->pad, item->dil, reinterpret_cast<hipStream_t>(stream), bn);
}

int lsn_conv2d_forward_prepared(int n_levels, const lsn_conv_level *levels, const void *prepared, const float *bias, int C,
                                int xpitch, int Co, int kh, int kw, int stride, int pad, int dil, int relu,
                                lsn_stream_t stream)
{
    return lsn::conv_forward_impl(n_levels, levels, prepared, bias, C, xpitch, Co, kh, kw, stride, pad, dil, relu,
                                  reinterpret_cast<hipStream_t>(stream));
}

int lsn_conv2d_backward_data_prepared(int n_levels, const lsn_conv_level *levels, const void *prepared, int C, int Co,
                                      int kh, int kw, int stride, int pad, int dil, lsn_stream_t stream)
{
    return lsn::conv_backward_data_impl(n_levels, levels, prepared, C, Co, kh, kw, stride, pad, dil,
                                        reinterpret_cast<hipStream_t>(stream));
}

// ---- one-shot forms: weight image built by the call (into `workspace`, or a stream-ordered temporary) ----
static int one_shot(int kind, int n_levels, const lsn_conv_level *levels, const float *w, const float *bias, void *workspace,
                    int C, int xpitch, int Co, int kh, int kw, int stride, int pad, int dil, int relu, lsn_stream_t stream)
{
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (!w) return lsn::fail(LSN_ERR_INVALID, "conv2d: weight is NULL");
    const int64_t bytes = lsn::prepared_bytes(kind, C, Co, kh, kw, stride, pad, dil);
    if (bytes < 0) return LSN_ERR_UNSUPPORTED;
    lsn::TempImage tmp(st);
    if (!workspace) {
        if (int rc = tmp.alloc((size_t)bytes)) return rc;
        workspace = tmp.p;
    }
    if (int rc = lsn::prepare_weights(kind, w, workspace, C, Co, kh, kw, stride, pad, dil, st)) return rc;
    if (kind == 0)
        return lsn::conv_forward_impl(n_levels, levels, workspace, bias, C, xpitch, Co, kh, kw, stride, pad, dil, relu, st);
    return lsn::conv_backward_data_impl(n_levels, levels, workspace, C, Co, kh, kw, stride, pad, dil, st);
}

int lsn_conv2d_forward_multi(int n_levels, const lsn_conv_level *levels, const float *w, const float *bias, void *workspace,
                             int C, int Co, int kh, int kw, int stride, int pad, int dil, int relu, lsn_stream_t stream)
{
    return one_shot(0, n_levels, levels, w, bias, workspace, C, C, Co, kh, kw, stride, pad, dil, relu, stream);
}

int lsn_conv2d_backward_data_multi(int n_levels, const lsn_conv_level *levels, const float *w, float *wt_workspace, int C,
                                   int Co, int kh, int kw, int stride, int pad, int dil, lsn_stream_t stream)
{
    return one_shot(1, n_levels, levels, w, nullptr, wt_workspace, C, C, Co, kh, kw, stride, pad, dil, 0, stream);
}

int lsn_conv2d_forward_pitched(const float *x, const float *w, const float *bias, float *out, void *workspace, int B,
                               int H, int W, int C, int xpitch, int Co, int kh, int kw, int stride, int pad, int dil,
                               int relu, lsn_stream_t stream)
{
    lsn_conv_level L = {};
    L.x = x, L.out = out, L.B = B, L.H = H, L.W = W;
    return one_shot(0, 1, &L, w, bias, workspace, C, xpitch, Co, kh, kw, stride, pad, dil, relu, stream);
}

int lsn_conv2d_forward(const float *x, const float *w, const float *bias, float *out, void *workspace, int B, int H,
                       int W, int C, int Co, int kh, int kw, int stride, int pad, int dil, int relu,
                       lsn_stream_t stream)
{
    return lsn_conv2d_forward_pitched(x, w, bias, out, workspace, B, H, W, C, C, Co, kh, kw, stride, pad, dil, relu, stream);
}

int lsn_conv2d_backward_data(const float *grad_out, const float *w, float *grad_in, float *wt_workspace, int B,
                             int H, int W, int C, int Co, int kh, int kw, int stride, int pad, int dil,
                             lsn_stream_t stream)
{
    lsn_conv_level L = {};
    L.x = grad_out, L.out = grad_in, L.B = B, L.H = H, L.W = W;
    return lsn_conv2d_backward_data_multi(1, &L, w, wt_workspace, C, Co, kh, kw, stride, pad, dil, stream);
}

}  // extern "C"
