// Host side of the deformable-convolution family: argument checks (mirroring the reference's
// TORCH_CHECKs, deform_conv_cuda.cpp:92-180,182-272), layout adapters, launch geometry and the
// extern "C" entry points declared in include/lsnet_hip.h.
#include <limits.h>
#include <string.h>

#include <vector>

#include "conv_route.h"
#include "dcn_kernels.h"
#include "dcn_mm_kernels.h"
#include "dcn_grouped_kernels.h"
#include "dcn_route.h"
#include "lib_state.h"
#include "prof.h"

namespace lsn {

// optional phase-clock capture and kernel routing for tests / A/B runs (diagnostics only; see lsn_debug_phase_clocks)
static long long *g_dbg_buf = nullptr;
static int g_dbg_block = 0;
static bool dbg_on(int bit) { return (g_dbg_block & bit) != 0; }   // bit: one of the LSN_DBG_* of lsnet_hip.h

static double dcn_flops(const DcnArgs &a)
{
    double px = 0;
    for (int i = 0; i < a.nlv; ++i) px += (double)a.lv[i].B * a.lv[i].Ho * a.lv[i].Wo;
    return 2.0 * px * a.Co * (a.C / a.groups) * a.kh * a.kw;
}

// algorithmic HBM bytes of one launch: every operand read or written once
static double dcn_bytes(const DcnArgs &a, int fam)
{
    const double K = (double)a.kh * a.kw;
    double in = 0, out = 0, om = 0;
    for (int i = 0; i < a.nlv; ++i) {
        const double opx = (double)a.lv[i].B * a.lv[i].Ho * a.lv[i].Wo;
        in += (double)a.lv[i].B * a.lv[i].H * a.lv[i].W * a.C;
        out += opx * a.Co;
        om += opx * a.dg * K * (a.lv[i].msk ? 3 : 2);
    }
    const double w = (double)a.Co * (a.C / a.groups) * K;
    switch (fam) {
    case PROF_FWD: return 4.0 * (in + om + w + out);
    case PROF_BWD_DATA: return 4.0 * (in + om + w + out + in + om);   // + grad_input, grad_offset/mask
    default: return 4.0 * (in + om + out + w);
    }
}

struct ProfScope : ProfSpan {
    ProfScope(int fam, const DcnArgs &a, hipStream_t s) : ProfSpan(fam, dcn_flops(a), dcn_bytes(a, fam), s) {}
};

// in[b][r][s] -> out[b][s][r]   (NCHW <-> NHWC with r = C, s = H*W; weight OIHW <-> OHWI with
// b = Co, r = Cg, s = kh*kw).  32x32 tiles through LDS so both sides are coalesced.
__global__ void permute_rs_kernel(const float *__restrict__ in, float *__restrict__ out, int R, int S)
{
    __shared__ float tile[32][33];
    const size_t base = (size_t)blockIdx.z * R * S;
    const int s0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int r = r0 + i, s = s0 + threadIdx.x;
        if (r < R && s < S) tile[i][threadIdx.x] = in[base + (size_t)r * S + s];
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int s = s0 + i, r = r0 + threadIdx.x;
        if (r < R && s < S) out[base + (size_t)s * R + r] = tile[threadIdx.x][i];
    }
}

static int permute_rs(const float *in, float *out, int Bn, int R, int S, hipStream_t st)
{
    if (Bn <= 0 || R <= 0 || S <= 0) return 0;
    for (int b0 = 0; b0 < Bn; b0 += 65535) {
        const int nb = Bn - b0 < 65535 ? Bn - b0 : 65535;
        dim3 grid(cdiv(S, 32), cdiv(R, 32), nb), block(32, 8);
        hipLaunchKernelGGL(permute_rs_kernel, grid, block, 0, st, in + (size_t)b0 * R * S,
                           out + (size_t)b0 * R * S, R, S);
    }
    LSN_HIP(hipGetLastError());
    return 0;
}

__global__ void scale_kernel(float *p, size_t n, float s)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        p[i] *= s;
}

// stream-ordered scratch: everything is freed (in stream order) when the holder goes out of scope
struct Scratch {
    hipStream_t st;
    std::vector<void *> ptrs;
    explicit Scratch(hipStream_t s) : st(s) {}
    float *get(size_t nfloats)
    {
        void *p = nullptr;
        if (nfloats == 0) nfloats = 1;
        if (hipMallocAsync(&p, nfloats * sizeof(float), st) != hipSuccess) return nullptr;
        lib_stat(STAT_POOL_ALLOCS, 1);
        ptrs.push_back(p);
        return reinterpret_cast<float *>(p);
    }
    ~Scratch()
    {
        for (void *p : ptrs) (void)hipFreeAsync(p, st);
    }
};

// The largest kh * kw * deformable_groups that every route of both passes serves (include/lsnet_hip.h LSN_DCN_KD_EVERY_ROUTE).
// Every kernel keeps the tap table of its 64-pixel tile in LDS, and the route moves on where a kernel's does not fit
// (dcn_route.h); the fp32 kernels come last, and of their tables the backward's is the larger: 44 bytes per (pixel, tap) beside
// the 8 KiB weight slab of its 64-wide tile.  Above this count, up to 64, a call is served where its route ends at another
// kernel and refused -- by the route, in front of every launch -- where it ends at the fp32 scatter.
constexpr int DCN_KD_EVERY_ROUTE = (int)((DR_LDS_MAX - bwd_fp32_lds(64, 0)) / (bwd_fp32_lds(64, 1) - bwd_fp32_lds(64, 0)));
static_assert(DCN_KD_EVERY_ROUTE == LSN_DCN_KD_EVERY_ROUTE, "include/lsnet_hip.h states this bound");
static_assert(bwd_fp32_lds(64, DCN_KD_EVERY_ROUTE) <= DR_LDS_MAX && bwd_fp32_lds(64, DCN_KD_EVERY_ROUTE + 1) > DR_LDS_MAX, "the bound");
static_assert(fwd_fp32_lds(64, 64) <= DR_LDS_MAX, "the forward pass serves every call check_shape admits");

static int check_shape(const lsn_dcn_shape &s)
{
    LSN_CHECK(s.kh > 0 && s.kw > 0, "kernel size should be greater than zero, but got kH: %d kW: %d", s.kh, s.kw);
    LSN_CHECK(s.stride > 0, "stride should be greater than zero, but got %d", s.stride);
    LSN_CHECK(s.dil > 0, "dilation should be greater than 0, but got %d", s.dil);
    LSN_CHECK(s.pad >= 0, "padding should be non-negative, but got %d", s.pad);
    LSN_CHECK(s.C > 0 && s.Co > 0, "channels must be positive (C %d, Co %d)", s.C, s.Co);
    LSN_CHECK(s.groups > 0 && s.C % s.groups == 0 && s.Co % s.groups == 0,
              "input/output channels (%d, %d) must be divisible by groups %d", s.C, s.Co, s.groups);
    LSN_CHECK(s.deformable_groups > 0 && s.C % s.deformable_groups == 0,
              "input channels must divide deformable group size");
    const int Cg = s.C / s.groups, cpdg = s.C / s.deformable_groups;
    if (!(Cg % cpdg == 0 || cpdg % Cg == 0))
        return fail(LSN_ERR_UNSUPPORTED, "groups %d / deformable_groups %d do not nest", s.groups,
                    s.deformable_groups);
    if (s.kh * s.kw * s.deformable_groups > 64)
        return fail(LSN_ERR_UNSUPPORTED, "kh*kw*deformable_groups = %d > 64 is not supported",
                    s.kh * s.kw * s.deformable_groups);
    LSN_CHECK(s.out_pitch == 0 || (s.out_pitch >= s.Co && s.out_pitch % 4 == 0),
              "out_pitch %d: 0 or a multiple of 4 >= Co = %d", s.out_pitch, s.Co);
    return 0;
}

static int i32(int64_t v, int *ok)
{
    if (v > INT_MAX || v < INT_MIN) *ok = 0;
    return (int)v;
}

template <typename KernelT>
static int set_lds(KernelT kernel, size_t bytes)
{
    if (bytes > 160 * 1024) return fail(LSN_ERR_UNSUPPORTED, "kernel needs %zu B of LDS (> 160 KiB)", bytes);
    if (bytes > 48 * 1024)
        LSN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}

// one launch of 256-thread workgroups with `lds` bytes of dynamic LDS
template <typename KernelT, typename... Args>
static int launch256(KernelT kern, dim3 grid, size_t lds, hipStream_t st, const Args &...args)
{
    if (int rc = set_lds(kern, lds)) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, args...);
    LSN_HIP(hipGetLastError());
    return 0;
}

// prow0 of every level, the launch-wide pixel-row numbering; returns the rows (the callers bound them)
static int number_rows(DcnArgs &a)
{
    int rows = 0;
    for (int i = 0; i < a.nlv; ++i) {
        a.lv[i].prow0 = rows;
        rows += a.lv[i].P;
    }
    return rows;
}

// tile0 of every level for tiles of `px` pixels; returns the tiles of the launch
static int number_tiles(DcnArgs &a, int px)
{
    int tiles = 0;
    for (int i = 0; i < a.nlv; ++i) {
        a.lv[i].tile0 = tiles;
        tiles += cdiv(a.lv[i].P, px);
    }
    return tiles;
}

// Fill the per-level part of DcnArgs from the public descriptors (NHWC pointers supplied here).
static int fill_levels(DcnArgs &a, const lsn_dcn_shape &s, int n, const lsn_dcn_level *lv, int tile_px)
{
    LSN_CHECK(n >= 1 && n <= MAXLV, "n_levels must be in [1,%d], got %d", MAXLV, n);
    int ok = 1, tiles = 0;
    for (int i = 0; i < n; ++i) {
        Lvl &L = a.lv[i];
        const lsn_dcn_level &d = lv[i];
        LSN_CHECK(d.B > 0 && d.H > 0 && d.W > 0 && d.Ho > 0 && d.Wo > 0,
                  "level %d: Given input size (%d x %d x %d), calculated output size (%d x %d x %d). "
                  "Output size is too small", i, s.C, d.H, d.W, s.Co, d.Ho, d.Wo);
        LSN_CHECK(d.offset != nullptr, "level %d: offset is NULL", i);
        L.B = d.B; L.H = d.H; L.W = d.W; L.Ho = d.Ho; L.Wo = d.Wo;
        L.P = i32((int64_t)d.B * d.Ho * d.Wo, &ok);
        (void)i32((int64_t)d.B * d.H * d.W * s.C, &ok);
        L.tile0 = tiles;
        tiles += cdiv(L.P, tile_px);
        L.sh = d.scale_h; L.sw = d.scale_w;
        L.off = d.offset; L.msk = d.mask;
        L.osb = i32(d.off_st.b, &ok); L.osc = i32(d.off_st.c, &ok);
        L.osh = i32(d.off_st.h, &ok); L.osw = i32(d.off_st.w, &ok);
        L.msb = i32(d.mask_st.b, &ok); L.msc = i32(d.mask_st.c, &ok);
        L.msh = i32(d.mask_st.h, &ok); L.msw = i32(d.mask_st.w, &ok);
        L.x = L.gout = nullptr;
        L.out = L.gx = nullptr;
        L.goff = d.grad_offset; L.gmsk = d.grad_mask;
    }
    if (!ok) return fail(LSN_ERR_UNSUPPORTED, "tensor too large for 32-bit indexing");
    a.nlv = n;
    a.ntiles = tiles;
    a.C = s.C; a.Co = s.Co; a.kh = s.kh; a.kw = s.kw; a.stride = s.stride; a.pad = s.pad; a.dil = s.dil;
    a.groups = s.groups; a.dg = s.deformable_groups;
    const int Cg = s.C / s.groups, cpdg = s.C / s.deformable_groups;
    a.SL = Cg < cpdg ? Cg : cpdg;
    a.msig = s.mask_is_logit ? 1 : 0;
    a.gcol = nullptr;
    a.gtap = nullptr;
    a.gtap_rows = 0;
    a.wg_vec = 0;
    a.mm = 0;   // (a field of the kernel argument that nothing reads any more: the route says which image wtp holds)
    a.opitch = s.out_pitch > 0 ? s.out_pitch : s.Co;
    a.wtp_bytes = 0;
    a.wg_part = a.wg_part_b = nullptr;
    a.dbg = g_dbg_buf;
    a.dbg_block = g_dbg_block;
    a.w = a.bias = nullptr;
    a.wtp = nullptr;
    a.gw = a.gb = nullptr;
    return 0;
}

// ---- the kernels of dcn_mm_kernels.h (dense-convolution skeleton): weight image, launches ----
static int mm_npl() { return split_npl(math_np()); }

// Work distribution of a forward launch (dcn_mm_kernels.h DcnSk): the stream-K pieces of conv_route.h under the deformable
// forward's own admission rule (sk_admit_dcn_fwd, with its measurements).
static DcnSk dcn_fwd_sk(int ntw, int Tall)
{
    const SkPieces p = sk_pieces(ntw, Tall, sk_admit_dcn_fwd(ntw, dbg_on(LSN_DBG_FWD_SK_ALWAYS), dbg_on(LSN_DBG_FWD_SK_NEVER)));
    return DcnSk{p.n_dp, p.sk_n, p.sk_tiles, nullptr, nullptr};
}

template <int TM, int TN, int WM, int WN, int NP, bool FINE = false>
static int launch_fwd_mm_cfg(const DcnArgs &a, hipStream_t st)
{
    constexpr int BN = WN * TN * 32;
    const size_t lds = dcn_fwd_mm_lds_bytes(SplitCfg<NP>::NPL, a.kh * a.kw * a.dg);
    const int blocks = a.ntiles * (a.Co / BN);
    DcnSk sk = dcn_fwd_sk(blocks, a.kh * a.kw * (a.C / 32));
    if (!sk.sk_n) return launch256(dcn_fwd_mm_kernel<TM, TN, WM, WN, NP, FINE, false>, dim3(blocks), lds, st, a, a.wtp, a.wtp_bytes, sk);
    if (int rc = stream_sk_scratch((size_t)2 * sk.sk_n * 64 * BN, &sk.part, &sk.cnt, st)) return rc;
    return launch256(dcn_fwd_mm_kernel<TM, TN, WM, WN, NP, FINE, true>, dim3(sk.n_dp + sk.sk_n), lds, st, a, a.wtp, a.wtp_bytes, sk);
}

static int launch_forward_mm(const DcnArgs &a, hipStream_t st)
{
    ProfScope prof(PROF_FWD, a, st);
    // (the 64 x 256 tile in the fine MFMA / staging interleave, dcn_mm_kernels.h FINE: tower launch 310 -> 280 us, pyramid
    // 818 -> 780 us in the round-4 A/B, profiles/r4_fine.txt)
    const bool wide = a.Co % 256 == 0;
    return split_dispatch(math_np(), [&](auto np) {
        constexpr int NP = decltype(np)::value;
        return wide ? launch_fwd_mm_cfg<2, 2, 1, 4, NP, true>(a, st) : launch_fwd_mm_cfg<1, 2, 2, 2, NP>(a, st);
    });
}

template <int BM, int BN, int WM, int WN>
static int launch_forward_t(const DcnArgs &a, bool vec, hipStream_t st)
{
    static_assert(BM == DR_FP32_BM, "dcn_route.h fwd_fp32_lds sizes this tile");
    const int Cog = a.Co / a.groups, KD = a.kh * a.kw * a.dg;
    const size_t lds = fwd_fp32_lds(BN, KD);   // (<= 160 KiB: route_forward)
    dim3 grid(a.ntiles, cdiv(Cog, BN), a.groups);
    return vec ? launch256(dcn_fwd_kernel<BM, BN, WM, WN, true>, grid, lds, st, a)
               : launch256(dcn_fwd_kernel<BM, BN, WM, WN, false>, grid, lds, st, a);
}

// ---- grouped calls (dcn_grouped_kernels.h): ResNeXt's 64 groups of 8 / 16 / 32 channels ----
static int launch_forward_grouped(const DcnArgs &a_in, hipStream_t st)
{
    DcnArgs a = a_in;
    a.ntiles = number_tiles(a, GF_PX);
    ProfScope prof(PROF_FWD, a, st);
    const size_t lds = dcn_fwd_grouped_lds_bytes(a.kh * a.kw);
    const dim3 grid(a.ntiles * (a.C / GF_CH));
    switch (a.C / a.groups) {
    case 8: return launch256(dcn_fwd_grouped_kernel<8>, grid, lds, st, a);
    case 16: return launch256(dcn_fwd_grouped_kernel<16>, grid, lds, st, a);
    default: return launch256(dcn_fwd_grouped_kernel<32>, grid, lds, st, a);
    }
}

// exact fp32 (LSN_MATH_FP32, narrow outputs, odd channel counts): the fp32-MFMA kernel with two workgroups per CU.
// bn: the route's tile (DcnRoute::fp32_bn) -- 256 output channels of a group, or 64 where a group has no more or the tap
// table leaves no room for the wide tile's weight slab
static int launch_forward_fp32(const DcnArgs &a, int bn, bool vec, hipStream_t st)
{
    ProfScope prof(PROF_FWD, a, st);
    return bn == 64 ? launch_forward_t<64, 64, 2, 2>(a, vec, st) : launch_forward_t<64, 256, 1, 4>(a, vec, st);
}

// planes: a.wtp holds the weights as dcn_prepare_w_kernel split them; otherwise every block splits its own
static int launch_forward_xn(const DcnArgs &a, bool planes, hipStream_t st)
{
    dim3 grid(a.ntiles, cdiv(a.Co / a.groups, PIPE_BN), a.groups);
    ProfScope prof(PROF_FWD, a, st);
    return split_dispatch(math_np(), [&](auto npc) {
        constexpr int NP = decltype(npc)::value;
        const size_t ldsn = xn_lds_bytes<NP>(a.kh * a.kw * a.dg);
        return planes ? launch256(dcn_fwd_xn_kernel<true, NP>, grid, ldsn, st, a) : launch256(dcn_fwd_xn_kernel<false, NP>, grid, ldsn, st, a);
    });
}

template <int RED>
static int launch_bwd_data_t(const DcnArgs &a, bool vec, hipStream_t st)
{
    const int KD = a.kh * a.kw * a.dg;
    const size_t lds = bwd_fp32_lds(RED, KD);   // (<= 160 KiB: route_backward)
    return vec ? launch256(dcn_bwd_data_kernel<RED, true>, dim3(a.ntiles), lds, st, a)
               : launch256(dcn_bwd_data_kernel<RED, false>, dim3(a.ntiles), lds, st, a);
}

// ---- the route of a call (dcn_route.h): the arguments as the shape the rule reads, and its plan as kernel arguments ----
static_assert(DR_MAXLV == MAXLV && DR_GT == GT && DR_GF_CH == GF_CH && DR_GC_COLS == GC_COLS, "dcn_route.h plans for these kernels");
static_assert(DR_WG_BP == WG_BP && DR_WG_BN == WG_BN && DR_WG_BM == WG_BM, "dcn_route.h counts the steps and tiles of these kernels");
static_assert(DR_TAP_BYTES == sizeof(Tap) && DR_GENTRY_BYTES == sizeof(GEntry), "dcn_route.h sizes the tables of these kernels");
static_assert(DR_FP32_BM == BWD_BM, "dcn_route.h sizes the tap tables of the fp32 kernels");

static size_t gather_ws_bytes(const lsn_dcn_shape &s) { return (size_t)(s.gather_workspace_bytes > 0 ? s.gather_workspace_bytes : 0); }
static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The only place that turns pointers into "present / aligned / shared" facts, and the only reader of the debug word and of the
// math mode on behalf of the rule.  want_wgrad: grad_weight is asked for (backward; the queries answer for the case they name).
static DcnRouteShape route_shape(const DcnArgs &a, const lsn_dcn_shape &s, lsn_layout layout, bool want_wgrad)
{
    DcnRouteShape r = {};
    r.n = a.nlv;
    for (int i = 0; i < a.nlv; ++i) {
        const Lvl &L = a.lv[i];
        DcnRouteLevel &R = r.lv[i];
        R.B = L.B, R.H = L.H, R.W = L.W, R.Ho = L.Ho, R.Wo = L.Wo, R.P = L.P;
        R.gx = L.gx != nullptr, R.goff = L.goff != nullptr, R.gmsk = L.gmsk != nullptr;
        R.x_aligned16 = aligned16(L.x), R.gout_aligned16 = aligned16(L.gout);
        R.gx_id = 0;
        while (a.lv[R.gx_id].gx != L.gx) ++R.gx_id;   // the first level with this buffer (i at the latest)
    }
    const int K = a.kh * a.kw, KD = K * a.dg;
    r.C = a.C, r.Co = a.Co, r.kh = a.kh, r.kw = a.kw, r.groups = a.groups, r.dg = a.dg, r.SL = a.SL, r.opitch = a.opitch;
    r.np = math_np(), r.npl = split_npl(r.np);
    r.nchw = layout == LSN_NCHW, r.want_wgrad = want_wgrad;
    r.workspace = s.workspace != nullptr;
    r.gather_ws = s.gather_workspace != nullptr, r.gather_ws_bytes = gather_ws_bytes(s);
    // (the rule asks this of the tap table, gather_workspace + plan.o_gtap: o_gtap is a multiple of 256, so it is the same test)
    r.gather_ws_aligned16 = aligned16(s.gather_workspace);
    r.general_gemms = dbg_on(LSN_DBG_GENERAL_GEMMS), r.atomic_scatter = dbg_on(LSN_DBG_ATOMIC_SCATTER);
    r.anchor_one_wave = dbg_on(LSN_DBG_ANCHOR_ONE_WAVE);
    r.fwd_mm_lds = dcn_fwd_mm_lds_bytes(r.npl, KD), r.xn_lds = xn_lds_bytes(r.npl, KD), r.bwd_xn_lds = bwd_xn_lds_bytes(r.np, KD);
    r.fwd_grouped_lds = dcn_fwd_grouped_lds_bytes(K);
    r.wfrag_fwd = cv_wfrag_bytes(a.Co, K, a.C, r.npl), r.wfrag_bwd = cv_wfrag_bytes(K * a.C, 1, a.Co, r.npl);
    return r;
}

// The plan as the kernels take it: prow0 / abase of the levels, and the groups with the pointers of the level that owns each
static void bind_plan(DcnArgs &a, const GatherPlan &pl, GatherArgs &ga, AnchorArgs &aa)
{
    for (int i = 0; i < a.nlv; ++i) a.lv[i].prow0 = pl.prow0[i], a.lv[i].abase = pl.abase[i];
    const int K = a.kh * a.kw, KD = K * a.dg;
    ga.ng = pl.nblk, ga.NB = pl.NB, ga.C = a.C, ga.K = K, ga.KD = KD, ga.dg = a.dg;
    aa.ng = pl.nanc, aa.NA = pl.NA, aa.C = a.C, aa.K = K, aa.KD = KD, aa.dg = a.dg;
    aa.ncb = pl.ncb, aa.hb_slot = pl.hb_slot;
    for (int j = 0; j < pl.nblk; ++j) {
        const GatherPlanGroup &G = pl.blk[j];
        ga.g[j] = GatherGrp{a.lv[G.level].gx, a.lv[G.level].x, G.B, G.H, G.W, G.abase, G.first};
    }
    for (int j = 0; j < pl.nanc; ++j) {
        const GatherPlanGroup &G = pl.anc[j];
        aa.g[j] = AnchorGrp{a.lv[G.level].gx, a.lv[G.level].x, G.B, G.H, G.W, G.abase, G.first};
    }
}

// x / grad_output / grad_input of a channels-last call, as the caller passes them (the callers check what they require)
static void bind_nhwc(DcnArgs &a, int n, const lsn_dcn_level *lv)
{
    for (int i = 0; i < n; ++i) a.lv[i].x = lv[i].input, a.lv[i].gout = lv[i].grad_output, a.lv[i].gx = lv[i].grad_input;
}

// Tap groups of the split backward-data GEMM (grid.y): the launch runs in ceil(tiles x groups / 512) rounds of the 512
// resident blocks (2 per CU) with blocks 1 / groups as long, plus a per-block prologue (gout tile -> registers, sampling
// table) of ~5 % of a whole tile (measured: 3 groups beat 9 on the tower launch): pick the divisor of K with the smallest
// rounds / groups x (1 + 0.05 groups).
static int bwd_tap_groups(const DcnArgs &a)
{
    const int K = a.kh * a.kw;
    int best = 1;
    double best_cost = 1e30;
    for (int g = 1; g <= K; ++g) {
        if (K % g) continue;
        const double cost = (double)cdiv(a.ntiles * g, 512) / g * (1.0 + 0.05 * g);
        if (cost < best_cost - 1e-9) best_cost = cost, best = g;
    }
    return best;
}

// A second stream per launch stream for the list building of the backward-data path.  The kernels of the list sort
// (build_lists) are short, latency-bound launches of a few hundred workgroups that depend on the offsets only; the
// column-gradient GEMM beside them depends on grad_output only and
// leaves ~100 VGPRs per SIMD and 110 KB of LDS per CU free.  Fork after the workspace is known, join before the
// per-anchor sums.  (Not the same experiment as the weight gradients on a side stream, profiles/r4_side_stream.txt: two
// MFMA kernels take the matrix pipe from each other; these kernels wait on memory while the GEMM computes.)
// (The TAIL of the path -- per-anchor sums, combine, offset gradients -- on this stream beside the weight-gradient pass of the
// same call was tried as well, profiles/r4_side_lists.txt: nothing on the tower launch, 995 vs 992 us per backward call (the
// gathers take the CUs from the weight gradient's workgroups instead of sharing them), -120 us on the pyramid launch,
// 0.25 ms per step -- and two kernel families that can no longer be timed apart.  Removed.)
struct SideStream {
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
};
static PerStream<SideStream> g_side;
static int side_stream(hipStream_t st, SideStream **out)
{
    return g_side.get(st, "side streams", out, [&](SideStream &S) {
        if (int rc = refuse_capture(st, "side stream would be created")) return rc;
        int lo = 0, hi = 0;
        LSN_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));   // hi = the numerically lowest = most urgent
        LSN_HIP(hipStreamCreateWithPriority(&S.side, hipStreamNonBlocking, hi));
        LSN_HIP(hipEventCreateWithFlags(&S.fork, hipEventDisableTiming));
        LSN_HIP(hipEventCreateWithFlags(&S.join, hipEventDisableTiming));
        return 0;
    });
}

// (Round 5 cut the launch into bands -- an anchor range per image of a grad_input map + the GEMM rows that scatter into it --
// and ran the per-anchor sums of band i on the side stream beside the GEMM of band i + 1, the column gradients of a band
// still in the Infinity Cache: tower +7 % slower, pyramid unchanged, profiles/r5_band_pipeline.txt.  GEMM and sums are both
// bound by the memory system; removed.)
// The sampling table (a.gtap, a.gtap_rows) and the anchor lists of a launch -- start[anchors + 1], ent[] -- on stream `st`:
// keys + low-digit histogram, then per pass scan and stable scatter (dcn_gather_kernels.h, dcn_sort_plan.h), then the list
// offsets.  Seven launches for up to 2^22 anchors (two passes), ten above; no memset, no blocking call.
static int build_lists(DcnArgs &a, const GatherPlan &pl, unsigned char *ws, hipStream_t st)
{
    int *hist = reinterpret_cast<int *>(ws + pl.o_hist), *start = reinterpret_cast<int *>(ws + pl.o_start);
    int *key = reinterpret_cast<int *>(ws + pl.o_key);
    int2 *pairs[2] = {reinterpret_cast<int2 *>(ws + pl.o_pairs), reinterpret_cast<int2 *>(ws + pl.o_pairs) + pl.nsamples};
    GEntry *ent = reinterpret_cast<GEntry *>(ws + pl.o_ent);
    Tap *gtap = reinterpret_cast<Tap *>(ws + pl.o_gtap);   // also read by the column-gradient kernels and by the weight-gradient pass
    const int KD = a.kh * a.kw * a.dg, n = pl.nsamples, na = pl.nanchors;
    a.gtap_rows = n / KD;
    const int db = ds_digit_bits(na), passes = ds_passes(na), nblocks = ds_blocks(n);
    const dim3 grid(nblocks), block(DS_THREADS), kblock(DS_KEY_THREADS);
    const size_t lds = ds_scatter_lds_bytes(db);   // (<= 40 KB: gather_plan)
    hipLaunchKernelGGL(dcn_list_keys_kernel, grid, kblock, 0, st, a, n, na, db, nblocks, key, hist, gtap);
    a.gtap = gtap;
    for (int p = 0; p < passes; ++p) {
        const int2 *in = p > 0 ? pairs[(p - 1) & 1] : nullptr;
        int2 *out = pairs[p & 1];
        if (p > 0) hipLaunchKernelGGL(dcn_list_hist_kernel, grid, kblock, 0, st, n, p, db, nblocks, in, hist);
        hipLaunchKernelGGL(dcn_list_scan_kernel, dim3(1 << db), block, 0, st, hist, db, nblocks);
        if (p == 0)
            hipLaunchKernelGGL((dcn_list_scatter_kernel<true, false>), grid, block, lds, st, n, na, p, db, nblocks, hist, key, in, out,
                               ent, (int *)nullptr, gtap, KD, a.gtap_rows);
        else if (p + 1 < passes)
            hipLaunchKernelGGL((dcn_list_scatter_kernel<false, false>), grid, block, lds, st, n, na, p, db, nblocks, hist, key, in, out,
                               ent, (int *)nullptr, gtap, KD, a.gtap_rows);
        else   // the last pass: entries, and the sorted keys where its pairs would have gone
            hipLaunchKernelGGL((dcn_list_scatter_kernel<false, true>), grid, block, lds, st, n, na, p, db, nblocks, hist, key, in,
                               (int2 *)nullptr, ent, reinterpret_cast<int *>(out), gtap, KD, a.gtap_rows);
    }
    const int *skey = reinterpret_cast<const int *>(pairs[(passes - 1) & 1]);
    hipLaunchKernelGGL(dcn_list_starts_kernel, dim3(cdiv(na + 1, 256)), dim3(256), 0, st, n, na, skey, start);
    LSN_HIP(hipGetLastError());
    return 0;
}

static int launch_bwd_gather(DcnArgs &a, const DcnRoute &r, unsigned char *ws, hipStream_t st_main)
{
    const GatherPlan &pl = r.plan;
    GatherArgs ga;
    AnchorArgs aa;
    bind_plan(a, pl, ga, aa);
    a.gcol = reinterpret_cast<float *>(ws + pl.o_gcol);
    int *start = reinterpret_cast<int *>(ws + pl.o_start);
    GEntry *ent = reinterpret_cast<GEntry *>(ws + pl.o_ent);
    // lists on the side stream only beside the dense GEMM (the other column-gradient kernels read the tap table)
    SideStream *side = nullptr;
    if (r.data == GATHER_MM)
        if (int rc = side_stream(st_main, &side)) return rc;
    hipStream_t st = side ? side->side : st_main;
    if (side) {
        LSN_HIP(hipEventRecord(side->fork, st_main));
        LSN_HIP(hipStreamWaitEvent(side->side, side->fork, 0));
    }
    if (int rc = build_lists(a, pl, ws, st)) return rc;
    if (side) {
        LSN_HIP(hipEventRecord(side->join, side->side));
        st = st_main;
    }
    bool any_off = false;
    for (int i = 0; i < a.nlv; ++i) any_off = any_off || a.lv[i].goff || a.lv[i].gmsk;
    float *Hb = nullptr;
    switch (r.data) {
    case GATHER_GROUPED:   // exact-fp32 column gradients per group, unweighted; the gather pass does the rest as for the dense GEMM
        if (r.gcol_ks) {
            DcnArgs g = a;
            const int nred = a.groups == 1 ? a.Co : GC_COLS;
            const size_t lds = dcn_gcol_mfma_lds_bytes(nred);
            const dim3 grid(number_tiles(g, GC_PX) * (a.C / GC_COLS));
            int rc = 0;
            switch (r.gcol_ks) {
            case 4: rc = launch256(dcn_gcol_mfma_kernel<4>, grid, lds, st, g, nred); break;
            case 8: rc = launch256(dcn_gcol_mfma_kernel<8>, grid, lds, st, g, nred); break;
            case 16: rc = launch256(dcn_gcol_mfma_kernel<16>, grid, lds, st, g, nred); break;
            case 32: rc = launch256(dcn_gcol_mfma_kernel<32>, grid, lds, st, g, nred); break;
            default: rc = launch256(dcn_gcol_mfma_kernel<64>, grid, lds, st, g, nred); break;
            }
            if (rc) return rc;
        } else {
            const long long nquads = (long long)pl.nsamples / a.dg * (a.C / 4);
            const int blocks = (int)((nquads + 255) / 256 < 16384 ? (nquads + 255) / 256 : 16384);
            hipLaunchKernelGGL(dcn_gcol_grouped_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, st, a, nquads);
        }
        if (any_off) Hb = reinterpret_cast<float *>(ws + pl.o_H);
        break;
    case GATHER_MM: {   // the dense kernel writes the unweighted column gradients; everything else happens in the gather pass
        const float *xs[MAXLV];
        float *outs[MAXLV];
        int rows[MAXLV];
        for (int i = 0; i < a.nlv; ++i) {
            xs[i] = a.lv[i].gout;
            outs[i] = a.gcol + (size_t)a.lv[i].prow0 * a.kh * a.kw * a.C;
            rows[i] = a.lv[i].P;
        }
        if (int rc = conv_mm_rows(a.nlv, xs, outs, rows, a.Co, a.opitch, a.kh * a.kw * a.C, a.wtp, st)) return rc;
        LSN_HIP(hipStreamWaitEvent(st_main, side->join, 0));
        if (any_off) Hb = reinterpret_cast<float *>(ws + pl.o_H);
        break;
    }
    default:   // GATHER_XN: mask-weighted column gradients, offset / mask gradients in the same kernel
        if (int rc = split_dispatch(math_np(), [&](auto npc) {
                constexpr int NP = decltype(npc)::value;
                return launch256(dcn_bwd_data_xn_kernel<NP, true>, dim3(a.ntiles, bwd_tap_groups(a)), bwd_xn_lds_bytes(NP, a.kh * a.kw * a.dg), st, a);
            }))
            return rc;
        break;
    }
    ga.raw = aa.raw = r.data != GATHER_XN ? 1 : 0;
    ga.Hb = aa.Hb = Hb;
    ga.gcol = a.gcol, ga.start = start, ga.ent = ent;
    if (aa.ng > 0) {   // per-anchor sums of all four corners, then four of them per pixel
        aa.gcol = a.gcol, aa.start = start, aa.ent = ent;
        aa.S = reinterpret_cast<float *>(ws + pl.o_S);
        if (pl.na_long > 0)
            hipLaunchKernelGGL(dcn_anchor_sum_kernel<4>, dim3(pl.na_long, aa.ncb), dim3(256), 0, st, aa, 0, pl.na_long);
        if (aa.NA > pl.na_long)
            hipLaunchKernelGGL(dcn_anchor_sum_kernel<1>, dim3(cdiv(aa.NA - pl.na_long, 4), aa.ncb), dim3(256), 0, st, aa,
                               pl.na_long, aa.NA - pl.na_long);
        hipLaunchKernelGGL(dcn_anchor_combine_kernel, dim3(cdiv(pl.anchor_pixels, 4)), dim3(256), 0, st, aa, pl.anchor_pixels);
    }
    if (ga.NB > 0) {
        // medium lists: four waves per pixel block; short ones (the tower launch, ~140 entries per block): one
        const bool split = pl.block_samples > (int64_t)300 * ga.NB;
        if (split)
            hipLaunchKernelGGL(dcn_gather_kernel<4>, dim3(ga.NB), dim3(256), 0, st, ga);
        else
            hipLaunchKernelGGL(dcn_gather_kernel<1>, dim3(cdiv(ga.NB, 4)), dim3(256), 0, st, ga);
    }
    if (Hb)
        hipLaunchKernelGGL(dcn_offgrad_kernel, dim3(cdiv(pl.nsamples, 256)), dim3(256), 0, st, a, pl.nsamples,
                           reinterpret_cast<const float4 *>(Hb), aa.ng > 0 ? aa.ncb : 1);
    LSN_HIP(hipGetLastError());
    return 0;
}

// gather_ws: the scratch the route's plan was sized for (GATHER_* only)
static int launch_bwd_data(DcnArgs &a, const DcnRoute &r, void *gather_ws, hipStream_t st)
{
    ProfScope prof(PROF_BWD_DATA, a, st);
    if (r.gather()) return launch_bwd_gather(a, r, reinterpret_cast<unsigned char *>(gather_ws), st);
    for (int i = 0; i < a.nlv; ++i)   // the scatter kernels accumulate: start from zero (once per buffer is enough)
        if (a.lv[i].gx)
            LSN_HIP(hipMemsetAsync(a.lv[i].gx, 0, sizeof(float) * (size_t)a.lv[i].B * a.lv[i].H * a.lv[i].W * a.C, st));
    if (r.data == SCATTER_XN)
        return split_dispatch(math_np(), [&](auto npc) {
            constexpr int NP = decltype(npc)::value;
            return launch256(dcn_bwd_data_xn_kernel<NP, false>, dim3(a.ntiles, bwd_tap_groups(a)), bwd_xn_lds_bytes(NP, a.kh * a.kw * a.dg), st, a);
        });
    return r.fp32_red == 256 ? launch_bwd_data_t<256>(a, r.vec, st) : launch_bwd_data_t<64>(a, r.vec, st);
}

// 8-byte buffer loads in the split weight-gradient kernel: even channel counts, 8-byte aligned tensors, byte offsets < 2^31
static int wgrad_vec_bits(const DcnArgs &a)
{
    bool vx = a.C % 2 == 0, vg = a.Co % 2 == 0;
    for (int i = 0; i < a.nlv; ++i) {
        const Lvl &L = a.lv[i];
        vx = vx && (reinterpret_cast<uintptr_t>(L.x) & 7) == 0 && (long long)L.B * L.H * L.W * a.C < (1ll << 29);
        vg = vg && (reinterpret_cast<uintptr_t>(L.gout) & 7) == 0 && (long long)(L.P + WG_BP) * a.Co < (1ll << 29);
    }
    return (vx ? 1 : 0) | (vg ? 2 : 0);
}

// ---- weight gradient on the kernels of dcn_mm_kernels.h: grad_output in fragment order, split partial tiles ----
// dense: a dense convolution's weight gradient (conv_wgrad_dense_mm: levels without offsets, no backward-data pass before this
// one): the sampling table is built here, the launch is accounted to the caller's family, the reduce applies the call's fold
static int launch_wgrad_mm(const DcnArgs &a_in, int nchunks, bool accumulate, hipStream_t st, const ConvWgradCall *dense = nullptr)
{
    DcnArgs a = a_in;
    const int K = a.kh * a.kw, npl = mm_npl();
    const size_t nW = (size_t)a.Co * K * a.C;
    const size_t img_bytes = (size_t)nchunks * 2 * (a.Co / 32) * npl * 1024;   // (< 2^31: wgrad_mm_image_ok)
    const int ncol = K * (a.C / 64), nz = a.Co / 256;
    int S = (512 + ncol * nz / 2) / (ncol * nz);
    if (S > nchunks / 4) S = nchunks / 4;   // a split should run long enough to amortise its prologue and its partial tile
    if (S < 1) S = 1;
    const int nsteps16 = 2 * nchunks;
    int spb = cdiv(nsteps16, 256);            // pre-pass: ~256 step ranges x (Co / 128) tile groups
    if (spb < 4) spb = 4;
    const int nblk_s = cdiv(nsteps16, spb);
    const size_t img_f = (img_bytes + 15) / 16 * 4, part_f = (size_t)S * nW, pb_f = ((size_t)nblk_s * a.Co + 3) & ~(size_t)3;
    const size_t meta_f = ((size_t)nchunks * 8 + 64 + 3) & ~(size_t)3;
    size_t tap_entries = 0;
    if (dense) {   // (< 2^26 entries, a 2 GB table: cw_dense_mm_ok)
        a.gtap_rows = number_rows(a);
        tap_entries = (size_t)a.gtap_rows * K * a.dg;
    }
    float *base = nullptr;
    if (int rc = wgrad_part_buffer(img_f + part_f + pb_f + meta_f + (tap_entries ? (tap_entries + 1) * (sizeof(Tap) / 4) : 0), &base, st))
        return rc;
    unsigned short *img = reinterpret_cast<unsigned short *>(base);
    float *part = base + img_f, *part_b = part + part_f;
    int *meta = reinterpret_cast<int *>(part_b + pb_f);
    if (dense) {
        Tap *tab = reinterpret_cast<Tap *>(part_b + pb_f + meta_f);
        const int n = (int)tap_entries > nchunks ? (int)tap_entries : nchunks;
        hipLaunchKernelGGL(dcn_tap_table_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, a, (int)tap_entries, tab, nchunks, meta);
        a.gtap = tab;
    } else {
        hipLaunchKernelGGL(dcn_chunk_meta_kernel, dim3(cdiv(nchunks, 256)), dim3(256), 0, st, a, nchunks, meta);
    }
    ProfScope prof(dense ? -1 : PROF_WGRAD, a, st);
    if (int rc = split_dispatch(math_np(), [&](auto np) {
            hipLaunchKernelGGL(dcn_gout_frag_kernel<SplitCfg<decltype(np)::value>::NPL>, dim3(nblk_s, a.Co / 128), dim3(256), 0, st, a,
                               nsteps16, spb, img, a.gb ? part_b : nullptr);
            return 0;
        }))
        return rc;
    const size_t lds = dcn_wgrad_mm_lds_bytes(npl);
    if ((long long)nchunks * (S + 1) >= (1ll << 32))
        return fail(LSN_ERR_UNSUPPORTED, "deformable backward-weight: %d chunks x %d splits exceed the kernel's 32-bit split arithmetic", nchunks, S);
    // (FINE = the fine MFMA / staging interleave: tower 360 -> 345 us, pyramid 941 -> 916 us, profiles/r4_fine.txt)
    if (int rc = split_dispatch(math_np(), [&](auto np) {
            constexpr int NP = decltype(np)::value;
            const dim3 grid(ncol, S, nz);
            return dense ? launch256(dcn_wgrad_mm_kernel<NP, true, true>, grid, lds, st, a, nchunks, img, (int)img_bytes, part, meta)
                         : launch256(dcn_wgrad_mm_kernel<NP, false, true>, grid, lds, st, a, nchunks, img, (int)img_bytes, part, meta);
        }))
        return rc;
    return conv_wgrad_reduce(part, a.gw, nW, part_b, a.gb, a.Co, S, nblk_s, accumulate ? 1 : 0, dense ? dense->fold : nullptr, st);
}

// grouped weight gradient (dcn_grouped_kernels.h): pixel splits leave partial tiles, the ordered reduce adds them (or queues)
static int launch_wgrad_grouped(const DcnArgs &a_in, bool accumulate, hipStream_t st)
{
    DcnArgs a = a_in;
    const int rows = number_rows(a);   // (the numbering of the backward-data pass's table, when there is one; < 2^30: route_backward)
    if ((reinterpret_cast<uintptr_t>(a.gtap) & 15) != 0 || a.gtap_rows != rows) a.gtap = nullptr;
    const int K = a.kh * a.kw, cg = a.C / a.groups;
    const int ny = (int)((int64_t)a.C * cg / 256);
    const int nch = cg >= 16 ? cg : 256 / cg, nco = 256 / cg;
    int splits = cdiv(3072, ny);                               // ~12 workgroups per CU: the kernel lives on loads in flight
    int per = cdiv(rows, splits);
    per = cdiv(per, GRP_PB) * GRP_PB;
    if (per < 4 * GRP_PB) per = 4 * GRP_PB;
    splits = cdiv(rows, per);
    const size_t nW = (size_t)a.Co * K * cg;
    const size_t cap = ((size_t)256 << 20) / 4 / (nW + a.Co);  // partial tiles: at most 256 MB
    if ((size_t)splits > cap) {
        splits = (int)(cap > 0 ? cap : 1);
        per = cdiv(cdiv(rows, splits), GRP_PB) * GRP_PB;
        splits = cdiv(rows, per);
    }
    float *base = nullptr;
    if (int rc = wgrad_part_buffer((size_t)splits * (nW + a.Co) + 16, &base, st)) return rc;
    float *part = base, *part_b = a.gb ? base + (((size_t)splits * nW + 3) & ~(size_t)3) : nullptr;
    ProfScope prof(PROF_WGRAD, a, st);
    const size_t lds = dcn_wgrad_grouped_lds_bytes(K, nch, nco);
    const dim3 grid(splits, ny);
    int rc;
    switch (cg) {
    case 4: rc = launch256(dcn_wgrad_grouped_kernel<4, 9>, grid, lds, st, a, rows, per, part, part_b); break;
    case 8: rc = launch256(dcn_wgrad_grouped_kernel<8, 9>, grid, lds, st, a, rows, per, part, part_b); break;
    case 16: rc = launch256(dcn_wgrad_grouped_kernel<16, 9>, grid, lds, st, a, rows, per, part, part_b); break;
    default: rc = launch256(dcn_wgrad_grouped_kernel<32, 9>, grid, lds, st, a, rows, per, part, part_b); break;
    }
    if (rc) return rc;
    return conv_wgrad_reduce(part, a.gw, nW, part_b, a.gb, a.Co, splits, splits, accumulate ? 1 : 0, nullptr, st);
}

// the split kernels (WG_XN_* / WG_FP32_*): ORDERED = one partial gradient per pixel split + an ordered reduce; a block that
// runs no step still stores its zero tile, so every partial element is written.  ATOMIC: fp32 atomics into the gradient.
static int launch_wgrad_split(const DcnArgs &a_in, const DcnRoute &r, bool accumulate, hipStream_t st)
{
    DcnArgs a = a_in;
    a.wg_vec = wgrad_vec_bits(a);
    if ((reinterpret_cast<uintptr_t>(a.gtap) & 15) != 0) a.gtap = nullptr;
    const int nsteps = r.wg_steps, ncol = r.wg_ncol, nz = r.wg_nz, splits = r.wg_splits;
    const size_t nW = (size_t)a.Co * a.kh * a.kw * (a.C / a.groups);
    const bool ordered = r.wgrad == WG_XN_ORDERED || r.wgrad == WG_FP32_ORDERED;
    if (ordered) {
        float *base = nullptr;
        if (int rc = wgrad_part_buffer((size_t)splits * (nW + a.Co) + 16, &base, st)) return rc;
        a.wg_part = base;
        a.wg_part_b = a.gb ? base + (((size_t)splits * nW + 3) & ~(size_t)3) : nullptr;
    } else if (!accumulate) {
        LSN_HIP(hipMemsetAsync(a.gw, 0, sizeof(float) * nW, st));
        if (a.gb) LSN_HIP(hipMemsetAsync(a.gb, 0, sizeof(float) * (size_t)a.Co, st));
    }
    ProfScope prof(PROF_WGRAD, a, st);
    const dim3 grid(ncol, splits, nz);
    int rc;
    if (r.wgrad == WG_FP32_ORDERED || r.wgrad == WG_FP32_ATOMIC) {   // exact fp32 (fp32 MFMA)
        const size_t lds = (size_t)WG_BP * (WG_BM + WG_BN) * 4 + 2 * WG_BP * sizeof(Tap);
        rc = r.vec ? launch256(dcn_wgrad_kernel<true>, grid, lds, st, a, nsteps) : launch256(dcn_wgrad_kernel<false>, grid, lds, st, a, nsteps);
    } else {
        rc = split_dispatch(math_np(), [&](auto np) {
            constexpr int NP = decltype(np)::value;
            return launch256(dcn_wgrad_xn_kernel<false, NP>, grid, wgrad_xn_lds_bytes<NP>(), st, a, nsteps);
        });
    }
    if (rc || !ordered) return rc;
    return conv_wgrad_reduce(a.wg_part, a.gw, nW, a.wg_part_b, a.gb, a.Co, splits, splits, accumulate ? 1 : 0, nullptr, st);
}

static int launch_wgrad(const DcnArgs &a, const DcnRoute &r, bool accumulate, hipStream_t st)
{
    DcnArgs w = a;   // same levels, step (32-pixel) indexing
    number_tiles(w, WG_BP);
    switch (r.wgrad) {
    case WG_GROUPED: return launch_wgrad_grouped(w, accumulate, st);
    case WG_MM: return launch_wgrad_mm(w, r.wg_steps, accumulate, st);
    default: return launch_wgrad_split(w, r, accumulate, st);
    }
}

// The weight image the route names, into the caller's `workspace`.  IMG_FRAGMENT: fragment order (forward: (Co, K, C) as it
// lies; backward: the transposed 1x1 view with N = K * C columns and the reduction over Co), already there with
// weights_prepared.  IMG_PLANES / IMG_PLANES_T: the split bf16 planes of dcn_kernels.h.
static int prepare_image(DcnArgs &a, WeightImage image, const lsn_dcn_shape &s, bool backward, hipStream_t st)
{
    if (image == IMG_NONE) return 0;
    unsigned short *dst = reinterpret_cast<unsigned short *>(s.workspace);
    const int K = a.kh * a.kw, np = math_np();
    WfragJob j = {};
    TapSub ts = {0, 1, 1, 0, 1, 1, 1};
    j.w = a.w, j.out = dst, j.Co = backward ? K * a.C : a.Co, j.K = backward ? 1 : K, j.C = backward ? a.Co : a.C;
    j.flipT = backward ? 1 : 0, j.ts = ts;
    const long long total = wfrag_threads(j);
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    if (int rc = split_dispatch(np, [&](auto npc) {
            constexpr int NPL = SplitCfg<decltype(npc)::value>::NPL;
            if (image == IMG_PLANES)
                hipLaunchKernelGGL(dcn_prepare_w_kernel<NPL>, dim3(512), dim3(256), 0, st, a.w, dst, (size_t)a.Co * K * (a.C / a.groups));
            else if (image == IMG_PLANES_T)
                hipLaunchKernelGGL(dcn_prepare_wt_kernel<NPL>, dim3(512), dim3(256), 0, st, a.w, dst, a.Co, K, a.C);
            else if (!s.weights_prepared)
                hipLaunchKernelGGL(conv_wfrag_kernel<NPL>, dim3(blocks), dim3(256), 0, st, j);
            return 0;
        }))
        return rc;
    LSN_HIP(hipGetLastError());
    a.wtp = dst;
    if (image == IMG_FRAGMENT) a.wtp_bytes = (int)cv_wfrag_bytes(j.Co, j.K, j.C, mm_npl());
    return 0;
}

static size_t n_in(const lsn_dcn_shape &s, const lsn_dcn_level &d) { return (size_t)d.B * s.C * d.H * d.W; }
static size_t n_out(const lsn_dcn_shape &s, const lsn_dcn_level &d) { return (size_t)d.B * s.Co * d.Ho * d.Wo; }

static int dcn_forward_impl(const lsn_dcn_shape &s, int n, const lsn_dcn_level *lv, const float *weight,
                            const float *bias, lsn_layout layout, hipStream_t st)
{
    if (int rc = check_shape(s)) return rc;
    LSN_CHECK(weight != nullptr, "weight is NULL");
    DcnArgs a;
    if (int rc = fill_levels(a, s, n, lv, 64)) return rc;
    Scratch ws(st);
    const int K = s.kh * s.kw, Cg = s.C / s.groups;
    std::vector<float *> out_tmp(n, nullptr), x_tmp(n, nullptr);
    float *w_tmp = nullptr;
    if (layout == LSN_NHWC) {
        a.w = weight;
        for (int i = 0; i < n; ++i) {
            LSN_CHECK(lv[i].input && lv[i].output, "level %d: input/output is NULL", i);
            a.lv[i].x = lv[i].input;
            a.lv[i].out = lv[i].output;
        }
    } else {
        // (channels-last temporaries: allocated here, filled behind the route's refusals)
        w_tmp = ws.get((size_t)s.Co * Cg * K);
        if (!w_tmp) return fail(LSN_ERR_RUNTIME, "workspace allocation failed");
        a.w = w_tmp;
        for (int i = 0; i < n; ++i) {
            LSN_CHECK(lv[i].input && lv[i].output, "level %d: input/output is NULL", i);
            x_tmp[i] = ws.get(n_in(s, lv[i]));
            out_tmp[i] = ws.get(n_out(s, lv[i]));
            if (!x_tmp[i] || !out_tmp[i]) return fail(LSN_ERR_RUNTIME, "workspace allocation failed");
            a.lv[i].x = x_tmp[i];
            a.lv[i].out = out_tmp[i];
        }
    }
    a.bias = bias;
    // the route, and every refusal it implies, in front of the first launch: a refused call has written nothing
    const DcnRoute r = route_forward(route_shape(a, s, layout, false));
    if (r.lds_over)
        return fail(LSN_ERR_UNSUPPORTED, "deformable forward: kh*kw*deformable_groups = %d needs %zu B of LDS (> 160 KiB) in the "
                    "fp32 kernel, the only one left for this call; every call with at most %d is served", K * s.deformable_groups,
                    r.lds_over, DCN_KD_EVERY_ROUTE);
    if (a.opitch != a.Co && !r.pitched)
        return fail(LSN_ERR_UNSUPPORTED, "deformable forward: out_pitch %d != Co %d outside the matrix-pipe kernels "
                    "(lsn_dcn_pitched_ok)", a.opitch, a.Co);
    if (s.weights_prepared && !r.prepared)
        return fail(LSN_ERR_UNSUPPORTED, "deformable forward: weights_prepared outside the matrix-pipe kernels (lsn_dcn_prepared_ok)");
    if (layout == LSN_NCHW) {
        if (int rc = permute_rs(weight, w_tmp, s.Co, Cg, K, st)) return rc;
        for (int i = 0; i < n; ++i)
            if (int rc = permute_rs(lv[i].input, x_tmp[i], lv[i].B, s.C, lv[i].H * lv[i].W, st)) return rc;
    }
    if (int rc = prepare_image(a, r.image, s, false, st)) return rc;
    int rc = 0;
    switch (r.fwd) {
    case FWD_MM: rc = launch_forward_mm(a, st); break;
    case FWD_GROUPED: rc = launch_forward_grouped(a, st); break;
    case FWD_XN_PLANES: rc = launch_forward_xn(a, true, st); break;
    case FWD_XN: rc = launch_forward_xn(a, false, st); break;
    case FWD_FP32: rc = launch_forward_fp32(a, r.fp32_bn, r.vec, st); break;
    }
    if (rc) return rc;
    if (layout == LSN_NCHW)
        for (int i = 0; i < n; ++i)
            if (int rc = permute_rs(out_tmp[i], lv[i].output, lv[i].B, lv[i].Ho * lv[i].Wo, s.Co, st)) return rc;
    return 0;
}

static int dcn_backward_impl(const lsn_dcn_shape &s, int n, const lsn_dcn_level *lv, const float *weight,
                             float *grad_weight, float *grad_bias, lsn_layout layout, hipStream_t st)
{
    if (int rc = check_shape(s)) return rc;
    LSN_CHECK(weight != nullptr, "weight is NULL");
    if (grad_bias && !grad_weight)
        return fail(LSN_ERR_UNSUPPORTED, "grad_bias without grad_weight is not supported");
    DcnArgs a;
    if (int rc = fill_levels(a, s, n, lv, BWD_BM)) return rc;
    Scratch ws(st);
    const int K = s.kh * s.kw, Cg = s.C / s.groups;
    std::vector<float *> gx_tmp(n, nullptr), x_tmp(n, nullptr), go_tmp(n, nullptr);
    float *gw_tmp = nullptr, *w_tmp = nullptr;
    for (int i = 0; i < n; ++i) LSN_CHECK(lv[i].input && lv[i].grad_output, "level %d: input/grad_output is NULL", i);
    if (layout == LSN_NHWC) {
        a.w = weight;
        a.gw = grad_weight;
        bind_nhwc(a, n, lv);
    } else {
        // (channels-last temporaries: allocated here, filled behind the route's refusals)
        w_tmp = ws.get((size_t)s.Co * Cg * K);
        if (!w_tmp) return fail(LSN_ERR_RUNTIME, "workspace allocation failed");
        a.w = w_tmp;
        if (grad_weight) {
            gw_tmp = ws.get((size_t)s.Co * Cg * K);
            if (!gw_tmp) return fail(LSN_ERR_RUNTIME, "workspace allocation failed");
            a.gw = gw_tmp;
        }
        for (int i = 0; i < n; ++i) {
            x_tmp[i] = ws.get(n_in(s, lv[i])), go_tmp[i] = ws.get(n_out(s, lv[i]));
            if (!x_tmp[i] || !go_tmp[i]) return fail(LSN_ERR_RUNTIME, "workspace allocation failed");
            a.lv[i].x = x_tmp[i];
            a.lv[i].gout = go_tmp[i];
            if (lv[i].grad_input) {
                gx_tmp[i] = ws.get(n_in(s, lv[i]));
                if (!gx_tmp[i]) return fail(LSN_ERR_RUNTIME, "workspace allocation failed");
                a.lv[i].gx = gx_tmp[i];
            }
        }
    }
    a.gb = grad_bias;

    void *gws = s.gather_workspace;
    // the route, and every refusal it implies, in front of the first launch: a refused call has written nothing
    const DcnRoute r = route_backward(route_shape(a, s, layout, a.gw != nullptr));
    if (r.lds_over)
        return fail(LSN_ERR_UNSUPPORTED, "deformable backward: kh*kw*deformable_groups = %d needs %zu B of LDS (> 160 KiB) in the "
                    "fp32 scatter kernel, the only one left for this call; every call with at most %d is served",
                    K * s.deformable_groups, r.lds_over, DCN_KD_EVERY_ROUTE);
    if (a.opitch != a.Co && r.data == DATA_NONE)
        return fail(LSN_ERR_UNSUPPORTED, "deformable backward: out_pitch without a data-gradient pass");
    if (a.opitch != a.Co && !r.pitched)
        return fail(LSN_ERR_UNSUPPORTED, "deformable backward: out_pitch %d != Co %d outside the matrix-pipe kernels "
                    "(lsn_dcn_pitched_ok)", a.opitch, a.Co);
    if (s.weights_prepared && r.data != DATA_NONE && !r.prepared)
        return fail(LSN_ERR_UNSUPPORTED, "deformable backward: weights_prepared outside the matrix-pipe kernels (lsn_dcn_prepared_ok)");
    if (layout == LSN_NCHW) {
        if (int rc = permute_rs(weight, w_tmp, s.Co, Cg, K, st)) return rc;
        for (int i = 0; i < n; ++i) {
            if (int rc = permute_rs(lv[i].input, x_tmp[i], lv[i].B, s.C, lv[i].H * lv[i].W, st)) return rc;
            if (int rc = permute_rs(lv[i].grad_output, go_tmp[i], lv[i].B, s.Co, lv[i].Ho * lv[i].Wo, st)) return rc;
        }
    }
    if (r.data != DATA_NONE) {
        if (r.own_gather_ws && !(gws = ws.get(r.plan.bytes / 4 + 64)))   // reference-layout entry points: own scratch
            return fail(LSN_ERR_RUNTIME, "workspace allocation failed");
        if (int rc = prepare_image(a, r.image, s, true, st)) return rc;
        if (int rc = launch_bwd_data(a, r, gws, st)) return rc;
    }
    // (the reference-layout path computes into a temporary that is permuted into grad_weight: no accumulation there)
    if (r.wgrad != WG_NONE)
        if (int rc = launch_wgrad(a, r, s.accumulate_param_grads != 0 && layout == LSN_NHWC, st)) return rc;
    if (layout == LSN_NCHW) {
        for (int i = 0; i < n; ++i)
            if (gx_tmp[i])
                if (int rc = permute_rs(gx_tmp[i], lv[i].grad_input, lv[i].B, lv[i].H * lv[i].W, s.C, st)) return rc;
        if (gw_tmp)
            if (int rc = permute_rs(gw_tmp, grad_weight, s.Co, K, Cg, st)) return rc;
    }
    return 0;
}

static lsn_strides4 nchw_strides(int Ch, int H, int W)
{
    lsn_strides4 s;
    s.b = (int64_t)Ch * H * W;
    s.c = (int64_t)H * W;
    s.h = W;
    s.w = 1;
    return s;
}

// shape + single NCHW level for the one-to-one wrappers
static int make_single(lsn_dcn_shape &s, lsn_dcn_level &L, int B, int C, int H, int W, int Co, int Ho, int Wo,
                       int kH, int kW, int dH, int dW, int padH, int padW, int dilH, int dilW, int group, int dg,
                       float scaleH, float scaleW, bool pyramid)
{
    if (dH != dW || padH != padW || dilH != dilW)
        return fail(LSN_ERR_UNSUPPORTED, "different stride/pad/dilation for h and w is not supported");
    memset(&s, 0, sizeof(s));
    memset(&L, 0, sizeof(L));
    LSN_CHECK(kH > 0 && kW > 0, "kernel size should be greater than zero, but got kH: %d kW: %d", kH, kW);
    LSN_CHECK(dH > 0, "stride should be greater than zero, but got dH: %d dW: %d", dH, dW);
    LSN_CHECK(dilH > 0, "dilation should be greater than 0, but got dilationH: %d dilationW: %d", dilH, dilW);
    if (!pyramid) {
        Ho = conv_out(H, kH, dH, padH, dilH);
        Wo = conv_out(W, kW, dW, padW, dilW);
    } else {
        // pyramid_shape_check: the output grid is derived from the OFFSET grid and must equal it
        LSN_CHECK(conv_out(Ho, kH, dH, padH, dilH) == Ho && conv_out(Wo, kW, dW, padW, dilW) == Wo,
                  "invalid spatial size of offset, expected height: %d width: %d, but got height: %d width: %d",
                  conv_out(Ho, kH, dH, padH, dilH), conv_out(Wo, kW, dW, padW, dilW), Ho, Wo);
    }
    LSN_CHECK(Ho >= 1 && Wo >= 1,
              "Given input size: (%d x %d x %d). Calculated output size: (%d x %d x %d). Output size is too small",
              C, H, W, Co, Ho, Wo);
    LSN_CHECK(H >= kH && W >= kW, "input image is smaller than kernel");
    s.B = B; s.C = C; s.H = H; s.W = W; s.Co = Co; s.Ho = Ho; s.Wo = Wo;
    s.kh = kH; s.kw = kW; s.stride = dH; s.pad = padH; s.dil = dilH;
    s.groups = group; s.deformable_groups = dg;
    s.scale_h = scaleH; s.scale_w = scaleW;
    L.B = B; L.H = H; L.W = W; L.Ho = Ho; L.Wo = Wo;
    L.scale_h = scaleH; L.scale_w = scaleW;
    L.off_st = nchw_strides(dg * 2 * kH * kW, Ho, Wo);
    L.mask_st = nchw_strides(dg * kH * kW, Ho, Wo);
    return 0;
}

// ---- the weight gradient of a dense convolution on this family's kernels (conv.hip validates, routes and accounts the call) ----
static_assert(CW_MAXLV <= MAXLV && CW_STEP_PX == WG_BP, "conv_wgrad_route.h counts the k-steps of these kernels");
bool general_gemms_only() { return dbg_on(LSN_DBG_GENERAL_GEMMS); }

// The levels of the call as DcnArgs (no offsets: the regular grid is the sampling table); returns the 32-pixel steps
static int conv_dcn_args(DcnArgs &a, const ConvWgradCall &c)
{
    const ConvWgradShape &s = c.s;
    a = DcnArgs{};
    int steps = 0;
    for (int i = 0; i < s.n; ++i) {
        Lvl &L = a.lv[i];
        L.x = c.x[i], L.gout = c.go[i];
        L.B = s.lv[i].B, L.H = s.lv[i].H, L.W = s.lv[i].W, L.Ho = s.lv[i].Ho, L.Wo = s.lv[i].Wo, L.P = s.lv[i].P, L.sh = L.sw = 1.f;
        L.tile0 = steps;
        steps += cdiv(L.P, WG_BP);
    }
    a.nlv = s.n;
    a.C = s.C, a.Co = s.Co, a.kh = s.kh, a.kw = s.kw, a.stride = s.stride, a.pad = c.pad, a.dil = s.dil, a.groups = 1, a.dg = 1;
    a.SL = s.C;
    a.opitch = s.Co;
    a.gw = c.gw, a.gb = c.gb;
    return steps;
}

int conv_wgrad_dense_mm(const ConvWgradCall &c, hipStream_t st)
{
    LSN_CHECK(cw_dense_mm_ok(c.s) && c.s.fold_jobs <= 1, "conv2d backward-weight: not a shape of the fragment-order kernel");
    DcnArgs a;
    const int steps = conv_dcn_args(a, c);
    return launch_wgrad_mm(a, steps, c.accumulate != 0, st, &c);
}

// dcn_wgrad_xn_kernel<PLAIN> (no offsets) with BMW output channels per workgroup
template <int NP, int BMW>
static int conv_wgrad_launch(DcnArgs a, int nsteps, const ConvWgradCall &c, hipStream_t st)
{
    const int C = a.C, Co = a.Co, K = a.kh * a.kw;
    const int ncc = cdiv(C, WG_BN), ncol = K * ncc, nz = cdiv(Co, BMW);
    int splits = wgrad_splits(ncol * nz, BMW == 256 ? 2 : 3);   // resident blocks per CU: registers (246 / 142 VGPRs)
    if (splits > nsteps) splits = nsteps;
    if (splits < 1) splits = 1;
    if (splits > 65535) splits = 65535;
    // one partial gradient per pixel split + an ordered reduce (deterministic) where the sizes allow; else fp32 atomics
    const size_t nW = (size_t)Co * K * C;
    const bool ordered = nW % 4 == 0 && (size_t)splits * (nW + Co) * sizeof(float) <= ((size_t)256 << 20);
    if (!ordered && c.fold)
        return fail(LSN_ERR_UNSUPPORTED, "conv2d backward-weight (folded norm): the gradient is too large for the ordered reduce");
    if (ordered) {
        float *base = nullptr;
        if (int rc = wgrad_part_buffer((size_t)splits * (nW + Co) + 16, &base, st)) return rc;
        a.wg_part = base;
        a.wg_part_b = a.gb ? base + (((size_t)splits * nW + 3) & ~(size_t)3) : nullptr;
    } else if (!c.accumulate) {
        LSN_HIP(hipMemsetAsync(a.gw, 0, sizeof(float) * nW, st));
        if (a.gb) LSN_HIP(hipMemsetAsync(a.gb, 0, sizeof(float) * (size_t)Co, st));
    }
    if (int rc = launch256(dcn_wgrad_xn_kernel<true, NP, BMW>, dim3(ncol, splits, nz), wgrad_xn_lds_bytes<NP, BMW>(), st, a, nsteps)) return rc;
    if (ordered) return conv_wgrad_reduce(a.wg_part, a.gw, nW, a.wg_part_b, a.gb, Co, splits, splits, c.accumulate, c.fold, st);
    return 0;
}

int conv_wgrad_general(const ConvWgradCall &c, hipStream_t st)
{
    LSN_CHECK(c.s.fold_jobs <= 1, "conv2d backward-weight: folded-norm jobs share a launch on the patch kernel only");
    DcnArgs a;
    const int steps = conv_dcn_args(a, c);
    a.wg_vec = wgrad_vec_bits(a);
    // exact-mode callers get the fp32-equivalent split: there is no fp32-MFMA dense wgrad
    return split_dispatch(c.s.np == 0 ? 6 : c.s.np, [&](auto npc) {
        constexpr int NP = decltype(npc)::value;
        return a.Co <= 64 ? conv_wgrad_launch<NP, 64>(a, steps, c, st) : conv_wgrad_launch<NP, 256>(a, steps, c, st);
    });
}

}  // namespace lsn

using namespace lsn;

extern "C" {

int lsn_debug_phase_clocks(long long *device_buf_512, int word)
{
    constexpr int known = LSN_DBG_BLOCK_MASK | LSN_DBG_ANCHOR_ONE_WAVE | LSN_DBG_FWD_SK_ALWAYS | LSN_DBG_FWD_SK_NEVER |
                          LSN_DBG_ATOMIC_SCATTER | LSN_DBG_WG_COMPUTED_TAPS | LSN_DBG_WG_SCALAR_LOADS | LSN_DBG_GENERAL_GEMMS;
    if (word & ~known) return fail(LSN_ERR_INVALID, "lsn_debug_phase_clocks: unknown debug bits 0x%x", (unsigned)(word & ~known));
    lsn::g_dbg_buf = device_buf_512;
    lsn::g_dbg_block = word;
    return 0;
}

// The queries: the shape of the arguments as a channels-last call binds them, then the route such a call would take
static bool query_shape(DcnRouteShape &rs, const lsn_dcn_shape *shape, int n_levels, const lsn_dcn_level *levels, int backward,
                        bool want_wgrad)
{
    using namespace lsn;
    DcnArgs a;
    if (!shape || !levels || check_shape(*shape) != 0) return false;
    if (fill_levels(a, *shape, n_levels, levels, backward ? BWD_BM : 64) != 0) return false;
    bind_nhwc(a, n_levels, levels);
    rs = route_shape(a, *shape, LSN_NHWC, want_wgrad);
    return true;
}

int64_t lsn_dcn_backward_workspace_bytes(const lsn_dcn_shape *shape, int n_levels, const lsn_dcn_level *levels)
{
    DcnRouteShape rs;
    if (!query_shape(rs, shape, n_levels, levels, 1, false)) return 0;
    // the answer is for a call that passes `workspace` and a gather workspace of this size
    rs.workspace = rs.gather_ws = true, rs.gather_ws_bytes = SIZE_MAX;
    const DcnRoute r = route_backward(rs);
    return r.gather() ? (int64_t)r.plan.bytes : 0;
}

int lsn_dcn_prepared_ok(const lsn_dcn_shape *shape, int n_levels, const lsn_dcn_level *levels, int backward)
{
    DcnRouteShape rs;
    if (!query_shape(rs, shape, n_levels, levels, backward, false)) return 0;
    return (backward ? route_backward(rs) : route_forward(rs)).prepared ? 1 : 0;
}

// (backward: the answer is for a call that asks for grad_weight)
int lsn_dcn_pitched_ok(const lsn_dcn_shape *shape, int n_levels, const lsn_dcn_level *levels, int backward)
{
    DcnRouteShape rs;
    if (!query_shape(rs, shape, n_levels, levels, backward, true)) return 0;
    return (backward ? route_backward(rs) : route_forward(rs)).pitched ? 1 : 0;
}

// (tests) the anchor lists lsn_dcn_backward would build for this call, and nothing else of it
int lsn_dcn_anchor_lists(const lsn_dcn_shape *shape, int n_levels, const lsn_dcn_level *levels, lsn_layout layout,
                         int *sample_anchor, int *list_start, int *list_sample, int64_t *counts, lsn_stream_t stream)
{
    using namespace lsn;
    if (!shape || !levels || !counts) return fail(LSN_ERR_INVALID, "shape/levels/counts is NULL");
    const lsn_dcn_shape &s = *shape;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (int rc = check_shape(s)) return rc;
    DcnArgs a;
    // (the reference-layout entry points route on temporaries of their own, which this entry does not make)
    if (layout != LSN_NHWC) return fail(LSN_ERR_UNSUPPORTED, "lsn_dcn_anchor_lists: LSN_NHWC only");
    if (int rc = fill_levels(a, s, n_levels, levels, BWD_BM)) return rc;
    for (int i = 0; i < n_levels; ++i) LSN_CHECK(levels[i].input && levels[i].grad_output, "level %d: input/grad_output is NULL", i);
    bind_nhwc(a, n_levels, levels);
    const DcnRoute r = route_backward(route_shape(a, s, layout, false));
    if (!r.gather()) return fail(LSN_ERR_UNSUPPORTED, "lsn_dcn_anchor_lists: this call builds no anchor lists (route without the gather pass)");
    const GatherPlan &pl = r.plan;
    counts[0] = pl.nsamples, counts[1] = pl.nanchors;
    if (!sample_anchor && !list_start && !list_sample) return 0;   // the sizes only
    LSN_CHECK(sample_anchor && list_start && list_sample, "lsn_dcn_anchor_lists: all three outputs or none");
    unsigned char *w = reinterpret_cast<unsigned char *>(s.gather_workspace);
    GatherArgs ga;   // (only the levels' part of the binding is used here)
    AnchorArgs aa;
    bind_plan(a, pl, ga, aa);
    if (int rc = build_lists(a, pl, w, st)) return rc;
    const int n = pl.nsamples > pl.nanchors + 1 ? pl.nsamples : pl.nanchors + 1;
    hipLaunchKernelGGL(dcn_list_export_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, pl.nsamples, pl.nanchors,
                       reinterpret_cast<const int *>(w + pl.o_key), reinterpret_cast<const int *>(w + pl.o_start),
                       reinterpret_cast<const GEntry *>(w + pl.o_ent), sample_anchor, list_start, list_sample);
    LSN_HIP(hipGetLastError());
    return 0;
}

int lsn_dcn_forward(const lsn_dcn_shape *shape, int n_levels, const lsn_dcn_level *levels, const float *weight,
                    const float *bias, lsn_layout layout, lsn_stream_t stream)
{
    if (!shape || !levels) return fail(LSN_ERR_INVALID, "shape/levels is NULL");
    return dcn_forward_impl(*shape, n_levels, levels, weight, bias, layout, stream);
}

int lsn_dcn_backward(const lsn_dcn_shape *shape, int n_levels, const lsn_dcn_level *levels, const float *weight,
                     float *grad_weight, float *grad_bias, lsn_layout layout, lsn_stream_t stream)
{
    if (!shape || !levels) return fail(LSN_ERR_INVALID, "shape/levels is NULL");
    return dcn_backward_impl(*shape, n_levels, levels, weight, grad_weight, grad_bias, layout, stream);
}

int lsn_deform_conv_forward(const float *input, const float *weight, const float *offset, float *output, int B,
                            int C, int H, int W, int Co, int kW, int kH, int dW, int dH, int padW, int padH,
                            int dilW, int dilH, int group, int deformable_group, int im2col_step,
                            lsn_stream_t stream)
{
    (void)im2col_step;
    lsn_dcn_shape s;
    lsn_dcn_level L;
    if (int rc = make_single(s, L, B, C, H, W, Co, 0, 0, kH, kW, dH, dW, padH, padW, dilH, dilW, group,
                             deformable_group, 1.f, 1.f, false))
        return rc;
    L.input = input; L.offset = offset; L.output = output;
    return dcn_forward_impl(s, 1, &L, weight, nullptr, LSN_NCHW, stream);
}

int lsn_deform_conv_backward_input(const float *input, const float *offset, const float *grad_output,
                                   float *grad_input, float *grad_offset, const float *weight, int B, int C,
                                   int H, int W, int Co, int kW, int kH, int dW, int dH, int padW, int padH,
                                   int dilW, int dilH, int group, int deformable_group, int im2col_step,
                                   lsn_stream_t stream)
{
    (void)im2col_step;
    lsn_dcn_shape s;
    lsn_dcn_level L;
    if (int rc = make_single(s, L, B, C, H, W, Co, 0, 0, kH, kW, dH, dW, padH, padW, dilH, dilW, group,
                             deformable_group, 1.f, 1.f, false))
        return rc;
    L.input = input; L.offset = offset; L.grad_output = grad_output;
    L.grad_input = grad_input; L.grad_offset = grad_offset;
    return dcn_backward_impl(s, 1, &L, weight, nullptr, nullptr, LSN_NCHW, stream);
}

static int scale_weight_grad(float *gw, size_t n, float scale, hipStream_t st)
{
    if (scale == 1.f) return 0;
    hipLaunchKernelGGL(scale_kernel, dim3(256), dim3(256), 0, st, gw, n, scale);
    LSN_HIP(hipGetLastError());
    return 0;
}

int lsn_deform_conv_backward_parameters(const float *input, const float *offset, const float *grad_output,
                                        float *grad_weight, int B, int C, int H, int W, int Co, int kW, int kH,
                                        int dW, int dH, int padW, int padH, int dilW, int dilH, int group,
                                        int deformable_group, float scale, int im2col_step, lsn_stream_t stream)
{
    (void)im2col_step;
    lsn_dcn_shape s;
    lsn_dcn_level L;
    if (int rc = make_single(s, L, B, C, H, W, Co, 0, 0, kH, kW, dH, dW, padH, padW, dilH, dilW, group,
                             deformable_group, 1.f, 1.f, false))
        return rc;
    L.input = input; L.offset = offset; L.grad_output = grad_output;
    // the weight values are not needed for dL/dW; pass grad_weight as a placeholder pointer
    if (int rc = dcn_backward_impl(s, 1, &L, grad_weight, grad_weight, nullptr, LSN_NCHW, stream)) return rc;
    return scale_weight_grad(grad_weight, (size_t)Co * (C / group) * kH * kW, scale, stream);
}

int lsn_modulated_deform_conv_forward(const float *input, const float *weight, const float *bias,
                                      const float *offset, const float *mask, float *output, int B, int C, int H,
                                      int W, int Co, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                      int pad_h, int pad_w, int dilation_h, int dilation_w, int group,
                                      int deformable_group, int with_bias, lsn_stream_t stream)
{
    lsn_dcn_shape s;
    lsn_dcn_level L;
    if (int rc = make_single(s, L, B, C, H, W, Co, 0, 0, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                             dilation_h, dilation_w, group, deformable_group, 1.f, 1.f, false))
        return rc;
    LSN_CHECK(mask != nullptr, "mask is NULL");
    L.input = input; L.offset = offset; L.mask = mask; L.output = output;
    return dcn_forward_impl(s, 1, &L, weight, with_bias ? bias : nullptr, LSN_NCHW, stream);
}

int lsn_modulated_deform_conv_backward(const float *input, const float *weight, const float *bias,
                                       const float *offset, const float *mask, float *grad_input,
                                       float *grad_weight, float *grad_bias, float *grad_offset, float *grad_mask,
                                       const float *grad_output, int B, int C, int H, int W, int Co, int kernel_h,
                                       int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                                       int dilation_h, int dilation_w, int group, int deformable_group,
                                       int with_bias, lsn_stream_t stream)
{
    (void)bias;
    lsn_dcn_shape s;
    lsn_dcn_level L;
    if (int rc = make_single(s, L, B, C, H, W, Co, 0, 0, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                             dilation_h, dilation_w, group, deformable_group, 1.f, 1.f, false))
        return rc;
    LSN_CHECK(mask != nullptr, "mask is NULL");
    L.input = input; L.offset = offset; L.mask = mask; L.grad_output = grad_output;
    L.grad_input = grad_input; L.grad_offset = grad_offset; L.grad_mask = grad_mask;
    return dcn_backward_impl(s, 1, &L, weight, grad_weight, with_bias ? grad_bias : nullptr, LSN_NCHW, stream);
}

int lsn_pyramid_deform_conv_forward(const float *input, const float *weight, const float *offset, float *output,
                                    int B, int C, int H, int W, int Co, int Ho, int Wo, int kW, int kH, int dW,
                                    int dH, int padW, int padH, int dilW, int dilH, float scaleW, float scaleH,
                                    int group, int deformable_group, int im2col_step, lsn_stream_t stream)
{
    (void)im2col_step;
    lsn_dcn_shape s;
    lsn_dcn_level L;
    if (int rc = make_single(s, L, B, C, H, W, Co, Ho, Wo, kH, kW, dH, dW, padH, padW, dilH, dilW, group,
                             deformable_group, scaleH, scaleW, true))
        return rc;
    L.input = input; L.offset = offset; L.output = output;
    return dcn_forward_impl(s, 1, &L, weight, nullptr, LSN_NCHW, stream);
}

int lsn_pyramid_deform_conv_backward_input(const float *input, const float *offset, const float *grad_output,
                                           float *grad_input, float *grad_offset, const float *weight, int B,
                                           int C, int H, int W, int Co, int Ho, int Wo, int kW, int kH, int dW,
                                           int dH, int padW, int padH, int dilW, int dilH, float scaleW,
                                           float scaleH, int group, int deformable_group, int im2col_step,
                                           lsn_stream_t stream)
{
    (void)im2col_step;
    lsn_dcn_shape s;
    lsn_dcn_level L;
    if (int rc = make_single(s, L, B, C, H, W, Co, Ho, Wo, kH, kW, dH, dW, padH, padW, dilH, dilW, group,
                             deformable_group, scaleH, scaleW, true))
        return rc;
    L.input = input; L.offset = offset; L.grad_output = grad_output;
    L.grad_input = grad_input; L.grad_offset = grad_offset;
    return dcn_backward_impl(s, 1, &L, weight, nullptr, nullptr, LSN_NCHW, stream);
}

int lsn_pyramid_deform_conv_backward_parameters(const float *input, const float *offset,
                                                const float *grad_output, float *grad_weight, int B, int C,
                                                int H, int W, int Co, int Ho, int Wo, int kW, int kH, int dW,
                                                int dH, int padW, int padH, int dilW, int dilH, float scaleW,
                                                float scaleH, int group, int deformable_group, float scale,
                                                int im2col_step, lsn_stream_t stream)
{
    (void)im2col_step;
    lsn_dcn_shape s;
    lsn_dcn_level L;
    if (int rc = make_single(s, L, B, C, H, W, Co, Ho, Wo, kH, kW, dH, dW, padH, padW, dilH, dilW, group,
                             deformable_group, scaleH, scaleW, true))
        return rc;
    L.input = input; L.offset = offset; L.grad_output = grad_output;
    if (int rc = dcn_backward_impl(s, 1, &L, grad_weight, grad_weight, nullptr, LSN_NCHW, stream)) return rc;
    return scale_weight_grad(grad_weight, (size_t)Co * (C / group) * kH * kW, scale, stream);
}

}  // extern "C"
