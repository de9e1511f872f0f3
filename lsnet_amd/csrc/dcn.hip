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

// 32-bit offsets: `elems` elements of `bytes_per` bytes stay below 2^31 (bytes_per = 1: a bound on the element count)
static bool fits_i32(int64_t elems, int bytes_per = 1) { return elems * bytes_per < ((int64_t)1 << 31); }
static int64_t in_elems(const DcnArgs &a, int i) { return (int64_t)a.lv[i].B * a.lv[i].H * a.lv[i].W * a.C; }
static int64_t col_elems(const DcnArgs &a, int i) { return (int64_t)a.lv[i].P * a.kh * a.kw * a.C; }   // column-gradient rows

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

// VEC kernels need 16-byte aligned float4 rows: channel counts that are multiples of 4
static bool vec_ok(const DcnArgs &a)
{
    const int Cg = a.C / a.groups, Cog = a.Co / a.groups;
    return (Cg % 4 == 0) && (Cog % 4 == 0) && (a.Co % 4 == 0) && (a.SL % 4 == 0);
}

// ---- the kernels of dcn_mm_kernels.h (dense-convolution skeleton): conditions, weight image, launches ----
static bool dcn_mm_env() { return !dbg_on(LSN_DBG_GENERAL_GEMMS); }   // (set: the kernels of dcn_kernels.h only -- tests, A/B runs)

static bool mm_common_ok(const DcnArgs &a)
{
    if (math_np() == 0 || a.groups != 1 || a.dg < 1 || a.C % a.dg != 0 || !dcn_mm_env()) return false;
    for (int i = 0; i < a.nlv; ++i)   // 32-bit buffer offsets
        if (!fits_i32(in_elems(a, i), 4) || !fits_i32((int64_t)a.lv[i].P * a.opitch, 4)) return false;
    return true;
}

static int mm_npl() { return split_npl(math_np()); }

static bool mm_fwd_ok(const DcnArgs &a)
{
    if (!mm_common_ok(a) || (a.C / a.dg) % 32 != 0 || a.Co % 128 != 0) return false;
    if (dcn_fwd_mm_lds_bytes(mm_npl(), a.kh * a.kw * a.dg) > 80 * 1024) return false;
    return fits_i32((int64_t)cv_wfrag_bytes(a.Co, a.kh * a.kw, a.C, mm_npl()));
}

// backward-data GEMM as a 1x1 convolution (conv.hip conv_mm_rows) + corner sums in the gather pass: every level that
// wants offset / mask gradients must also want grad_input (its samples are then on the anchor lists); the fragment image
// has to fit the caller's weight workspace (8 bytes per weight element, include/lsnet_hip.h)
static bool mm_bwd_ok(const DcnArgs &a)
{
    if (!mm_common_ok(a) || a.C % 4 != 0 || a.Co % 4 != 0) return false;
    for (int i = 0; i < a.nlv; ++i)
        if ((a.lv[i].goff || a.lv[i].gmsk) && !a.lv[i].gx) return false;
    const size_t wb = cv_wfrag_bytes(a.kh * a.kw * a.C, 1, a.Co, mm_npl());
    return fits_i32((int64_t)wb) && wb <= (size_t)8 * a.Co * a.kh * a.kw * a.C;
}

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
static int launch_forward_t(const DcnArgs &a, hipStream_t st)
{
    const int Cog = a.Co / a.groups, KD = a.kh * a.kw * a.dg;
    const size_t lds = (size_t)(BM + BN) * 33 * 4 + (size_t)BM * KD * sizeof(Tap);
    dim3 grid(a.ntiles, cdiv(Cog, BN), a.groups);
    return vec_ok(a) ? launch256(dcn_fwd_kernel<BM, BN, WM, WN, true>, grid, lds, st, a)
                     : launch256(dcn_fwd_kernel<BM, BN, WM, WN, false>, grid, lds, st, a);
}

// the split one-workgroup-per-CU kernel (dcn_fwd_xn_kernel) needs float4 rows and 32-bit byte offsets into x and w
static bool xn_ok(const DcnArgs &a)
{
    if (a.Co / a.groups <= 64 || !vec_ok(a)) return false;
    if (!fits_i32((int64_t)a.Co * a.kh * a.kw * (a.C / a.groups), 4)) return false;
    for (int i = 0; i < a.nlv; ++i)
        if (!fits_i32(in_elems(a, i), 4)) return false;
    return true;
}

// ---- grouped calls (dcn_grouped_kernels.h): ResNeXt's 64 groups of 8 / 16 / 32 channels ----
static bool grouped_inputs_ok(const DcnArgs &a)   // 16-byte loads at 32-bit element offsets
{
    for (int i = 0; i < a.nlv; ++i)
        if (!fits_i32(in_elems(a, i)) || (reinterpret_cast<uintptr_t>(a.lv[i].x) & 15) != 0) return false;
    return true;
}

static bool grouped_fwd_ok(const DcnArgs &a)
{
    if (a.groups <= 1 || a.C % a.groups != 0 || a.Co != a.C) return false;
    const int cg = a.C / a.groups;
    if (!(cg == 8 || cg == 16 || cg == 32) || a.C % GF_CH != 0 || a.C % a.dg != 0 || (a.C / a.dg) % GF_CH != 0) return false;
    return dcn_fwd_grouped_lds_bytes(a.kh * a.kw) <= 64 * 1024 && grouped_inputs_ok(a);
}

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

// exact fp32 (LSN_MATH_FP32, narrow outputs, odd channel counts): the fp32-MFMA kernel with two workgroups per CU
static int launch_forward_fp32(const DcnArgs &a, hipStream_t st)
{
    ProfScope prof(PROF_FWD, a, st);
    return (a.Co / a.groups <= 64) ? launch_forward_t<64, 64, 2, 2>(a, st) : launch_forward_t<64, 256, 1, 4>(a, st);
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
static int launch_bwd_data_t(const DcnArgs &a, hipStream_t st)
{
    const int KD = a.kh * a.kw * a.dg;
    const size_t lds = (size_t)RED * 32 * 4 + (size_t)BWD_BM * KD * (sizeof(Tap) + 12);
    return vec_ok(a) ? launch256(dcn_bwd_data_kernel<RED, true>, dim3(a.ntiles), lds, st, a)
                     : launch256(dcn_bwd_data_kernel<RED, false>, dim3(a.ntiles), lds, st, a);
}

// 32-bit buffer offsets into the input and into every level's column-gradient rows (backward-data, every kernel in front
// of the gather pass)
static bool bwd_offsets_ok(const DcnArgs &a)
{
    for (int i = 0; i < a.nlv; ++i)
        if (!fits_i32(in_elems(a, i), 4) || !fits_i32(col_elems(a, i), 4)) return false;
    return true;
}

// round 2's split GEMM (dcn_bwd_data_xn_kernel) on the transposed weight planes the caller's `workspace` holds
static bool bwd_x3_ok(const DcnArgs &a)
{
    if (math_np() == 0 || a.groups != 1) return false;
    if (a.Co > 256 || a.Co % 8 != 0 || a.C % 4 != 0) return false;
    if (!fits_i32((int64_t)a.kh * a.kw * a.C * a.Co, 6)) return false;
    if (bwd_xn_lds_bytes(math_np(), a.kh * a.kw * a.dg) > 80 * 1024) return false;
    return bwd_offsets_ok(a);
}

static bool bwd_colbuf_env() { return !dbg_on(LSN_DBG_ATOMIC_SCATTER); }   // (set: the atomic scatter kernels -- tests)

// Exact-fp32 column gradients (dcn_gcol_grouped_kernel: fmaf chains per group) in front of the gather pass: grouped calls
// (config 4: 64 groups) in every math mode, and -- round 6 -- EVERY call of LSN_MATH_FP32: the exact mode used to scatter
// with fp32 atomics (round 1's kernels) and was the less reproducible, less exact of the modes; it now
// shares the atomic-free, bit-reproducible gather with the default mode and differs from it in the GEMM arithmetic only.
// Levels that want offset / mask gradients must want grad_input (anchor lists).
static bool bwd_grouped_ok(const DcnArgs &a)
{
    if (a.groups <= 1 && math_np() != 0) return false;
    if (a.C % a.groups != 0 || a.Co % a.groups != 0 || (a.C / a.groups) % 4 != 0 || a.C % a.dg != 0) return false;
    if ((a.C / a.dg) % 4 != 0 || !bwd_colbuf_env()) return false;
    for (int i = 0; i < a.nlv; ++i)
        if ((a.lv[i].goff || a.lv[i].gmsk) && !a.lv[i].gx) return false;
    return bwd_offsets_ok(a);
}

// ---- atomic-free grad_input: workspace plan of the list sort / gather sequence (dcn_gather_kernels.h) ----
struct GatherPlan {
    bool ok = false;
    int nsamples = 0, nanchors = 0;
    size_t o_gcol = 0, o_hist = 0, o_start = 0, o_key = 0, o_ent = 0, o_gtap = 0, bytes = 0;
    size_t o_S = 0, o_H = 0, o_pairs = 0;
    GatherArgs ga;        // groups gathered per 4x4 pixel block
    AnchorArgs aa;        // groups with long lists: gathered per anchor (dcn_anchor_sum / combine)
    int anchor_pixels = 0;
    int na_long = 0;             // the first na_long anchors of the S buffer belong to long-list groups (4 waves each)
    int64_t block_samples = 0;   // samples (upper bound) of the block-gathered groups
};

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Fills prow0 / abase of the levels and the plan.  gx pointers: levels with the same grad_input share an anchor grid.
// all_anchor: every group on the per-anchor path (route_backward says when).
static void gather_plan(DcnArgs &a, GatherPlan &pl, bool all_anchor)
{
    pl.ok = false;
    const int K = a.kh * a.kw, KD = K * a.dg;
    int64_t prow = 0, anchors = 0, Q = 0;
    GatherArgs &ga = pl.ga;
    ga.ng = 0;
    bool any = false;
    int64_t gsamp[MAXLV] = {};   // samples (upper bound: every tap valid) that scatter into each group
    for (int i = 0; i < a.nlv; ++i) {
        Lvl &L = a.lv[i];
        L.prow0 = (int)prow;
        prow += L.P;
        L.abase = 0;
        if (!L.gx) continue;
        any = true;
        int gi = -1;
        for (int j = 0; j < ga.ng; ++j)
            if (ga.g[j].gx == L.gx) gi = j;
        if (gi < 0) {
            gi = ga.ng++;
            GatherGrp &G = ga.g[gi];
            G.gx = L.gx, G.x = L.x, G.B = L.B, G.H = L.H, G.W = L.W;
            G.abase = (int)anchors, G.blk0 = (int)Q;
            anchors += (int64_t)L.B * (L.H + 1) * (L.W + 1);
            Q += (int64_t)L.B * cdiv(L.H, GT) * cdiv(L.W, GT);
        } else if (ga.g[gi].B != L.B || ga.g[gi].H != L.H || ga.g[gi].W != L.W) {
            return;   // one buffer, two shapes: not a valid call for this path
        }
        L.abase = ga.g[gi].abase;
        gsamp[gi] += (int64_t)L.P * KD;
    }
    if (!any) return;
    if (prow * KD >= ((int64_t)1 << 30) || anchors >= ((int64_t)1 << 30) || Q >= ((int64_t)1 << 30)) return;
    if (a.C % 4 != 0 || (a.C / a.dg) % 4 != 0) return;
    pl.nsamples = (int)(prow * KD);
    pl.nanchors = (int)anchors;
    if (ds_digit_bits(pl.nanchors) > DS_MAX_DIGIT_BITS) return;   // (cannot happen below 2^30 anchors: the LDS of the list sort)
    // Groups with more than ~400 samples per 4x4 pixel block go to the per-anchor gather (the pyramid op's coarse source
    // levels); the others keep the block walk.
    constexpr int anchor_thr = 400;
    AnchorArgs &aa = pl.aa;
    aa.ng = 0, aa.NA = 0;
    pl.anchor_pixels = 0, pl.block_samples = 0;
    {
        // anchor path: every group when the unweighted-GEMM pipeline can serve the call (its corner sums are cheapest per
        // anchor), otherwise the groups above the threshold.  Long-list groups first: they get four waves per anchor.
        GatherGrp keep[MAXLV];
        bool to_anchor[MAXLV], is_long[MAXLV];
        int nk = 0;
        int64_t q = 0;
        for (int j = 0; j < ga.ng; ++j) {
            const GatherGrp &G = ga.g[j];
            const int64_t nblk = (int64_t)G.B * cdiv(G.H, GT) * cdiv(G.W, GT);
            const int64_t nanch = (int64_t)G.B * (G.H + 1) * (G.W + 1);
            to_anchor[j] = all_anchor || (anchor_thr > 0 && gsamp[j] > (int64_t)anchor_thr * nblk);
            constexpr int long_thr = 40;
            is_long[j] = !all_anchor || gsamp[j] > (int64_t)long_thr * nanch;   // mean list length (upper bound)
        }
        for (int pass = 0; pass < 2; ++pass) {
            for (int j = 0; j < ga.ng; ++j) {
                const GatherGrp &G = ga.g[j];
                if (!to_anchor[j] || is_long[j] != (pass == 0)) continue;
                AnchorGrp &A = aa.g[aa.ng++];
                A.gx = G.gx, A.x = G.x, A.B = G.B, A.H = G.H, A.W = G.W, A.abase = G.abase, A.a0 = aa.NA;
                aa.NA += G.B * (G.H + 1) * (G.W + 1);
                pl.anchor_pixels += G.B * G.H * G.W;
            }
            if (pass == 0) pl.na_long = aa.NA;
        }
        for (int j = 0; j < ga.ng; ++j) {
            if (to_anchor[j]) continue;
            const GatherGrp &G = ga.g[j];
            keep[nk] = G;
            keep[nk].blk0 = (int)q;
            q += (int64_t)G.B * cdiv(G.H, GT) * cdiv(G.W, GT);
            pl.block_samples += gsamp[j];
            ++nk;
        }
        for (int j = 0; j < nk; ++j) ga.g[j] = keep[j];
        ga.ng = nk;
        Q = q;
    }
    ga.NB = (int)Q;
    ga.C = a.C, ga.K = K, ga.KD = KD, ga.dg = a.dg;
    aa.C = a.C, aa.K = K, aa.KD = KD, aa.dg = a.dg;
    size_t o = 0;
    pl.o_gcol = o, o = align256(o + (size_t)prow * K * a.C * sizeof(float));
    // the histogram of one pass, [digit][block] + the digits' totals: (blocks + 1) x 2^db ints with 2^db <= 2 sqrt(anchors),
    // i.e. at most 4 bytes per sample + 16 sqrt(anchors) -- less than the anchor counters and sample ranks it replaces
    pl.o_hist = o, o = align256(o + ds_hist_ints(pl.nsamples, pl.nanchors) * sizeof(int));
    pl.o_start = o, o = align256(o + ((size_t)pl.nanchors + 1) * sizeof(int));
    pl.o_key = o, o = align256(o + (size_t)pl.nsamples * sizeof(int));
    pl.o_ent = o, o = align256(o + (size_t)pl.nsamples * sizeof(GEntry));
    pl.o_gtap = o, o = align256(o + ((size_t)pl.nsamples + 1) * sizeof(Tap));   // + the all-zero entry
    pl.o_S = o, o = align256(o + (size_t)pl.aa.NA * 4 * a.C * sizeof(float));
    // corner sums (dcn_offgrad_kernel): one slot per 256-channel block where the per-anchor sums split them over blockIdx.y
    // (every group on the per-anchor path, C > 256; dcn_gather_kernels.h AnchorArgs::ncb)
    // (LSN_DBG_ANCHOR_ONE_WAVE: one wave walks all blocks of its anchor, the form until round 6 -- tests; the workspace is sized for
    // the split either way, so a size asked for under one setting serves a launch under the other)
    const int ncb_max = (ga.NB == 0 && aa.ng > 0 && a.C > 256) ? cdiv(a.C, 256) : 1;
    aa.ncb = dbg_on(LSN_DBG_ANCHOR_ONE_WAVE) ? 1 : ncb_max;
    aa.hb_slot = (long long)pl.nsamples * 4;
    pl.o_H = o, o = align256(o + (size_t)pl.nsamples * 4 * sizeof(float) * ncb_max);
    pl.o_pairs = o, o = align256(o + (size_t)pl.nsamples * 2 * sizeof(int2));   // the (key, sample) pairs of the sort, ping and pong
    pl.bytes = o;
    pl.ok = true;
}

// Pixel splits of a weight-gradient launch: the grid (columns x splits x co blocks) fills ONE round of the blocks the chip
// holds at once (256 CUs x per_cu), rounded DOWN.  Measured on the benchmark step (profiles/r2_wgrad_rounds.txt): the
// old cdiv(1024, 36) = 29 splits made 1044 blocks = two full rounds plus a third with 20 blocks (0.88 ms per DCN
// launch); 28 splits 0.68 ms; one round instead of two is the same for the DCN launches and 1.1 ms / step faster over
// the dense layers (half the fp32 atomics of the epilogues).
static int wgrad_splits(int cols, int per_cu)
{
    const int slots = 256 * per_cu;
    int s = slots / cols;
    return s < 1 ? 1 : s;
}

// weight gradient on the kernels of dcn_mm_kernels.h (it also needs the tap table of the gather pass: route_backward)
static bool mm_wgrad_ok(const DcnArgs &a) { return mm_common_ok(a) && a.Co % 256 == 0 && (a.C / a.dg) % 64 == 0; }
// ... and its fragment-order image of grad_output (nchunks 32-pixel chunks) at 32-bit byte offsets
static bool wgrad_mm_image_ok(const DcnArgs &a, int nchunks) { return fits_i32((int64_t)nchunks * 2 * (a.Co / 32) * mm_npl(), 1024); }

static bool grouped_wgrad_ok(const DcnArgs &a)
{
    if (a.groups <= 1 || a.C % a.groups != 0 || a.Co != a.C || a.kh * a.kw > 9) return false;
    const int cg = a.C / a.groups;
    if (!(cg == 4 || cg == 8 || cg == 16 || cg == 32) || ((int64_t)a.C * cg) % 256 != 0 || a.C % a.dg != 0) return false;
    const int nch = cg >= 16 ? cg : 256 / cg;
    if ((a.C / a.dg) % nch != 0 || a.C % nch != 0) return false;
    return grouped_inputs_ok(a);
}

// ---- the route of a call: which kernel serves each pass and what else that fixes.  route_forward / route_backward decide
// it once, before anything is launched; they are the only callers of the *_ok predicates and of gather_plan, and the three
// queries of the C ABI (lsn_dcn_backward_workspace_bytes, lsn_dcn_prepared_ok, lsn_dcn_pitched_ok) read their answers. ----
enum FwdKernel { FWD_MM, FWD_GROUPED, FWD_XN_PLANES, FWD_XN, FWD_FP32 };
// GATHER_*: column gradients from that kernel, then the atomic-free gather pass; SCATTER_*: fp32 atomics into grad_input
enum DataKernel { DATA_NONE, GATHER_GROUPED, GATHER_MM, GATHER_XN, SCATTER_XN, SCATTER_FP32 };
enum WgradKernel { WG_NONE, WG_GROUPED, WG_MM, WG_XN_ORDERED, WG_XN_ATOMIC, WG_FP32_ORDERED, WG_FP32_ATOMIC };
// what the caller's `workspace` gets: nothing, the fragment-order image of dcn_mm_kernels.h (the only one a caller may
// hand over prepared), the split bf16 planes (forward) or the split and transposed ones (backward)
enum WeightImage { IMG_NONE, IMG_FRAGMENT, IMG_PLANES, IMG_PLANES_T };

struct DcnRoute {
    FwdKernel fwd = FWD_FP32;
    DataKernel data = DATA_NONE;
    WgradKernel wgrad = WG_NONE;
    WeightImage image = IMG_NONE;
    bool pitched = false;    // out_pitch != Co is served (lsn_dcn_pitched_ok)
    bool prepared = false;   // weights_prepared is served (lsn_dcn_prepared_ok)
    int gcol_ks = 0;         // GATHER_GROUPED: k-steps of dcn_gcol_mfma_kernel; 0: the fmaf chains of dcn_gcol_grouped_kernel
    int wg_steps = 0;        // weight gradient: 32-pixel steps of all levels
    bool own_gather_ws = false;        // LSN_NCHW without the caller's gather workspace: plan.bytes of the call's own scratch
    GatherPlan plan;                   // GATHER_*: computed here, once
    bool gather() const { return data == GATHER_GROUPED || data == GATHER_MM || data == GATHER_XN; }
};

// Order: mm -> grouped -> xn -> fp32.  The reference-layout (LSN_NCHW) entry points take the same kernels but neither
// out_pitch nor a prepared image.
static DcnRoute route_forward(const DcnArgs &a, const lsn_dcn_shape &s, lsn_layout layout)
{
    DcnRoute r;
    const int np = math_np();
    if (s.workspace && mm_fwd_ok(a)) {
        r.fwd = FWD_MM, r.image = IMG_FRAGMENT;
    } else if (grouped_fwd_ok(a)) {
        r.fwd = FWD_GROUPED;
    } else if (np != 0 && xn_ok(a) && xn_lds_bytes(split_npl(np), a.kh * a.kw * a.dg) <= 160 * 1024) {
        r.fwd = FWD_XN;   // with a workspace the weights are split once instead of in every block
        if (s.workspace && (a.C / a.groups) % 8 == 0) r.fwd = FWD_XN_PLANES, r.image = IMG_PLANES;
    }
    r.pitched = r.prepared = layout == LSN_NHWC && r.fwd == FWD_MM;
    return r;
}

// k-steps of the fp32-MFMA column gradients (dcn_grouped_kernels.h dcn_gcol_mfma_kernel); 0: the fmaf-chain kernel
static int gcol_mfma_ksteps(const DcnArgs &a)
{
    const int Cg = a.C / a.groups, Cog = a.Co / a.groups;
    if (a.C % GC_COLS != 0 || a.opitch % 4 != 0) return 0;
    for (int i = 0; i < a.nlv; ++i)
        if ((reinterpret_cast<uintptr_t>(a.lv[i].gout) & 15) != 0) return 0;
    if (a.groups == 1) return (a.Co == 64 || a.Co == 128 || a.Co == 256) ? a.Co / 4 : 0;
    return (Cog == Cg && (Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32)) ? (Cg == 32 ? 8 : 4) : 0;
}

// grid of the split weight-gradient kernels (dcn_wgrad_kernel / dcn_wgrad_xn_kernel): columns, co blocks; returns the pixel splits
static int wgrad_split_grid(const DcnArgs &a, int nsteps, int *ncol, int *nz)
{
    const int K = a.kh * a.kw, Cg = a.C / a.groups, Cog = a.Co / a.groups;
    *ncol = a.groups * K * (Cg / a.SL) * cdiv(a.SL, WG_BN), *nz = cdiv(Cog, WG_BM);
    int s = wgrad_splits(*ncol * *nz, 2);   // 2 resident blocks per CU (246 VGPRs, 78 KB LDS)
    if (s > nsteps) s = nsteps;
    if (s < 1) s = 1;
    return s > 65535 ? 65535 : s;
}

// gws / gws_bytes: the caller's gather workspace.  want_wgrad: grad_weight is asked for (the queries answer for that case).
// Backward-data: the gather path where a column-gradient kernel serves the call -- grouped (groups > 1, or any call of
// LSN_MATH_FP32), else mm, else xn -- and a gather workspace holds the plan; else scatter xn; else the fp32 scatter.
// Weight gradient: grouped (dense grad_output, 4 | weight elements) -> mm (reads the gather pass's tap table) -> the split
// kernels.  A prepared image is served by GATHER_MM (so: groups = 1, a split-bf16 mode, even Co, some data gradient), out_pitch
// by GATHER_MM and -- when grad_weight is asked for -- WG_MM; neither by the reference-layout (LSN_NCHW) entry points, which
// get the call's own gather scratch instead of the caller's.
static DcnRoute route_backward(DcnArgs &a, const lsn_dcn_shape &s, lsn_layout layout, const void *gws, size_t gws_bytes,
                               bool want_wgrad)
{
    DcnRoute r;
    const int np = math_np(), K = a.kh * a.kw;
    bool any_data = false;
    for (int i = 0; i < a.nlv; ++i) any_data = any_data || a.lv[i].gx || a.lv[i].goff || a.lv[i].gmsk;
    if (any_data) {
        // can_split: `workspace` gets a bf16 image of the weights (8 bytes per weight element: even Co for the planes)
        const bool can_split = s.workspace && np && a.groups == 1 && a.Co % 2 == 0;
        const bool grouped = bwd_grouped_ok(a), mm = mm_bwd_ok(a), x3 = can_split && bwd_x3_ok(a);
        const DataKernel cand = !bwd_colbuf_env()                         ? DATA_NONE
                                : grouped                                 ? GATHER_GROUPED
                                : (can_split && mm && bwd_offsets_ok(a)) ? GATHER_MM
                                : x3                                      ? GATHER_XN
                                                                          : DATA_NONE;
        bool fits = false;
        if (cand != DATA_NONE && (gws || layout == LSN_NCHW)) {
            // (all_anchor keys on what the arguments admit, not on the kernel taken: the workspace size a caller asked for
            // without `workspace` serves the call with it)
            gather_plan(a, r.plan, mm || grouped);
            r.own_gather_ws = !gws && r.plan.ok;
            fits = r.plan.ok && (r.own_gather_ws || r.plan.bytes <= gws_bytes);
        }
        r.data = fits ? cand : x3 ? SCATTER_XN : SCATTER_FP32;
        if (r.data == GATHER_GROUPED) r.gcol_ks = gcol_mfma_ksteps(a);
        // (the transposed planes are written for every call that can split, also where the fp32 scatter then ignores them)
        r.image = r.data == GATHER_MM ? IMG_FRAGMENT : can_split ? IMG_PLANES_T : IMG_NONE;
        r.prepared = layout == LSN_NHWC && r.data == GATHER_MM;
    }
    if (want_wgrad) {
        int64_t rows = 0, steps = 0;
        for (int i = 0; i < a.nlv; ++i) rows += a.lv[i].P, steps += cdiv(a.lv[i].P, WG_BP);
        r.wg_steps = (int)steps;
        const size_t nW = (size_t)a.Co * K * (a.C / a.groups);
        // the tap table of the gather pass, 16-byte aligned (the call's own scratch is)
        const bool tap_table = r.gather() && (r.own_gather_ws || ((reinterpret_cast<uintptr_t>(gws) + r.plan.o_gtap) & 15) == 0);
        if (grouped_wgrad_ok(a) && a.opitch == a.Co && nW % 4 == 0 && rows < ((int64_t)1 << 30)) {
            r.wgrad = WG_GROUPED;
        } else if (mm_wgrad_ok(a) && tap_table && wgrad_mm_image_ok(a, r.wg_steps)) {
            r.wgrad = WG_MM;
        } else {
            // one partial gradient per pixel split + an ordered reduce instead of fp32 atomics (deterministic) where they fit
            int ncol, nz;
            const int splits = wgrad_split_grid(a, r.wg_steps, &ncol, &nz);
            const bool ordered = nW % 4 == 0 && (size_t)splits * (nW + a.Co) * sizeof(float) <= ((size_t)256 << 20);
            r.wgrad = np ? (ordered ? WG_XN_ORDERED : WG_XN_ATOMIC) : (ordered ? WG_FP32_ORDERED : WG_FP32_ATOMIC);
        }
    }
    r.pitched = layout == LSN_NHWC && r.data == GATHER_MM && (!want_wgrad || r.wgrad == WG_MM);
    return r;
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

static int launch_bwd_gather(DcnArgs &a, DcnRoute &r, unsigned char *ws, hipStream_t st_main)
{
    GatherPlan &pl = r.plan;
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
    pl.ga.raw = pl.aa.raw = r.data != GATHER_XN ? 1 : 0;
    pl.ga.Hb = pl.aa.Hb = Hb;
    pl.ga.gcol = a.gcol, pl.ga.start = start, pl.ga.ent = ent;
    if (pl.aa.ng > 0) {   // per-anchor sums of all four corners, then four of them per pixel
        pl.aa.gcol = a.gcol, pl.aa.start = start, pl.aa.ent = ent;
        pl.aa.S = reinterpret_cast<float *>(ws + pl.o_S);
        if (pl.na_long > 0)
            hipLaunchKernelGGL(dcn_anchor_sum_kernel<4>, dim3(pl.na_long, pl.aa.ncb), dim3(256), 0, st, pl.aa, 0, pl.na_long);
        if (pl.aa.NA > pl.na_long)
            hipLaunchKernelGGL(dcn_anchor_sum_kernel<1>, dim3(cdiv(pl.aa.NA - pl.na_long, 4), pl.aa.ncb), dim3(256), 0, st, pl.aa,
                               pl.na_long, pl.aa.NA - pl.na_long);
        hipLaunchKernelGGL(dcn_anchor_combine_kernel, dim3(cdiv(pl.anchor_pixels, 4)), dim3(256), 0, st, pl.aa, pl.anchor_pixels);
    }
    if (pl.ga.NB > 0) {
        // medium lists: four waves per pixel block; short ones (the tower launch, ~140 entries per block): one
        const bool split = pl.block_samples > (int64_t)300 * pl.ga.NB;
        if (split)
            hipLaunchKernelGGL(dcn_gather_kernel<4>, dim3(pl.ga.NB), dim3(256), 0, st, pl.ga);
        else
            hipLaunchKernelGGL(dcn_gather_kernel<1>, dim3(cdiv(pl.ga.NB, 4)), dim3(256), 0, st, pl.ga);
    }
    if (Hb)
        hipLaunchKernelGGL(dcn_offgrad_kernel, dim3(cdiv(pl.nsamples, 256)), dim3(256), 0, st, a, pl.nsamples,
                           reinterpret_cast<const float4 *>(Hb), pl.aa.ng > 0 ? pl.aa.ncb : 1);
    LSN_HIP(hipGetLastError());
    return 0;
}

// gather_ws: the scratch the route's plan was sized for (GATHER_* only)
static int launch_bwd_data(DcnArgs &a, DcnRoute &r, void *gather_ws, hipStream_t st)
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
    return (a.Co / a.groups > 64) ? launch_bwd_data_t<256>(a, st) : launch_bwd_data_t<64>(a, st);
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
    const int nsteps = r.wg_steps;
    int ncol, nz;
    const int splits = wgrad_split_grid(a, nsteps, &ncol, &nz);
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
        rc = vec_ok(a) ? launch256(dcn_wgrad_kernel<true>, grid, lds, st, a, nsteps) : launch256(dcn_wgrad_kernel<false>, grid, lds, st, a, nsteps);
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

static size_t gather_ws_bytes(const lsn_dcn_shape &s) { return (size_t)(s.gather_workspace_bytes > 0 ? s.gather_workspace_bytes : 0); }
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
    std::vector<float *> out_tmp(n, nullptr);
    if (layout == LSN_NHWC) {
        a.w = weight;
        for (int i = 0; i < n; ++i) {
            LSN_CHECK(lv[i].input && lv[i].output, "level %d: input/output is NULL", i);
            a.lv[i].x = lv[i].input;
            a.lv[i].out = lv[i].output;
        }
    } else {
        float *w2 = ws.get((size_t)s.Co * Cg * K);
        if (!w2) return fail(LSN_ERR_RUNTIME, "workspace allocation failed");
        if (int rc = permute_rs(weight, w2, s.Co, Cg, K, st)) return rc;
        a.w = w2;
        for (int i = 0; i < n; ++i) {
            LSN_CHECK(lv[i].input && lv[i].output, "level %d: input/output is NULL", i);
            float *x2 = ws.get(n_in(s, lv[i]));
            out_tmp[i] = ws.get(n_out(s, lv[i]));
            if (!x2 || !out_tmp[i]) return fail(LSN_ERR_RUNTIME, "workspace allocation failed");
            if (int rc = permute_rs(lv[i].input, x2, lv[i].B, s.C, lv[i].H * lv[i].W, st)) return rc;
            a.lv[i].x = x2;
            a.lv[i].out = out_tmp[i];
        }
    }
    a.bias = bias;
    const DcnRoute r = route_forward(a, s, layout);
    if (a.opitch != a.Co && !r.pitched)
        return fail(LSN_ERR_UNSUPPORTED, "deformable forward: out_pitch %d != Co %d outside the matrix-pipe kernels "
                    "(lsn_dcn_pitched_ok)", a.opitch, a.Co);
    if (s.weights_prepared && !r.prepared)
        return fail(LSN_ERR_UNSUPPORTED, "deformable forward: weights_prepared outside the matrix-pipe kernels (lsn_dcn_prepared_ok)");
    if (int rc = prepare_image(a, r.image, s, false, st)) return rc;
    int rc = 0;
    switch (r.fwd) {
    case FWD_MM: rc = launch_forward_mm(a, st); break;
    case FWD_GROUPED: rc = launch_forward_grouped(a, st); break;
    case FWD_XN_PLANES: rc = launch_forward_xn(a, true, st); break;
    case FWD_XN: rc = launch_forward_xn(a, false, st); break;
    case FWD_FP32: rc = launch_forward_fp32(a, st); break;
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
    std::vector<float *> gx_tmp(n, nullptr);
    float *gw_tmp = nullptr;
    for (int i = 0; i < n; ++i) LSN_CHECK(lv[i].input && lv[i].grad_output, "level %d: input/grad_output is NULL", i);
    if (layout == LSN_NHWC) {
        a.w = weight;
        a.gw = grad_weight;
        for (int i = 0; i < n; ++i) {
            a.lv[i].x = lv[i].input;
            a.lv[i].gout = lv[i].grad_output;
            a.lv[i].gx = lv[i].grad_input;
        }
    } else {
        float *w2 = ws.get((size_t)s.Co * Cg * K);
        if (!w2) return fail(LSN_ERR_RUNTIME, "workspace allocation failed");
        if (int rc = permute_rs(weight, w2, s.Co, Cg, K, st)) return rc;
        a.w = w2;
        if (grad_weight) {
            gw_tmp = ws.get((size_t)s.Co * Cg * K);
            if (!gw_tmp) return fail(LSN_ERR_RUNTIME, "workspace allocation failed");
            a.gw = gw_tmp;
        }
        for (int i = 0; i < n; ++i) {
            float *x2 = ws.get(n_in(s, lv[i])), *g2 = ws.get(n_out(s, lv[i]));
            if (!x2 || !g2) return fail(LSN_ERR_RUNTIME, "workspace allocation failed");
            if (int rc = permute_rs(lv[i].input, x2, lv[i].B, s.C, lv[i].H * lv[i].W, st)) return rc;
            if (int rc = permute_rs(lv[i].grad_output, g2, lv[i].B, s.Co, lv[i].Ho * lv[i].Wo, st)) return rc;
            a.lv[i].x = x2;
            a.lv[i].gout = g2;
            if (lv[i].grad_input) {
                gx_tmp[i] = ws.get(n_in(s, lv[i]));
                if (!gx_tmp[i]) return fail(LSN_ERR_RUNTIME, "workspace allocation failed");
                a.lv[i].gx = gx_tmp[i];
            }
        }
    }
    a.gb = grad_bias;

    void *gws = s.gather_workspace;
    DcnRoute r = route_backward(a, s, layout, gws, gather_ws_bytes(s), a.gw != nullptr);
    if (a.opitch != a.Co && r.data == DATA_NONE)
        return fail(LSN_ERR_UNSUPPORTED, "deformable backward: out_pitch without a data-gradient pass");
    if (a.opitch != a.Co && !r.pitched)
        return fail(LSN_ERR_UNSUPPORTED, "deformable backward: out_pitch %d != Co %d outside the matrix-pipe kernels "
                    "(lsn_dcn_pitched_ok)", a.opitch, a.Co);
    if (s.weights_prepared && r.data != DATA_NONE && !r.prepared)
        return fail(LSN_ERR_UNSUPPORTED, "deformable backward: weights_prepared outside the matrix-pipe kernels (lsn_dcn_prepared_ok)");
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
bool general_gemms_only() { return !dcn_mm_env(); }

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

// The queries: the arguments as a channels-last call binds them, then the route such a call would take
static bool query_args(lsn::DcnArgs &a, const lsn_dcn_shape *shape, int n_levels, const lsn_dcn_level *levels, int backward)
{
    using namespace lsn;
    if (!shape || !levels || check_shape(*shape) != 0) return false;
    if (fill_levels(a, *shape, n_levels, levels, backward ? BWD_BM : 64) != 0) return false;
    for (int i = 0; i < n_levels; ++i) {
        a.lv[i].x = levels[i].input;
        a.lv[i].gout = levels[i].grad_output;
        a.lv[i].gx = levels[i].grad_input;
    }
    return true;
}

int64_t lsn_dcn_backward_workspace_bytes(const lsn_dcn_shape *shape, int n_levels, const lsn_dcn_level *levels)
{
    using namespace lsn;
    DcnArgs a;
    if (!query_args(a, shape, n_levels, levels, 1)) return 0;
    lsn_dcn_shape s = *shape;
    s.workspace = &s;   // any non-NULL value: the answer is for a call that passes `workspace` and a gather workspace of this size
    const DcnRoute r = route_backward(a, s, LSN_NHWC, &s, SIZE_MAX, false);
    return r.gather() ? (int64_t)r.plan.bytes : 0;
}

int lsn_dcn_prepared_ok(const lsn_dcn_shape *shape, int n_levels, const lsn_dcn_level *levels, int backward)
{
    using namespace lsn;
    DcnArgs a;
    if (!query_args(a, shape, n_levels, levels, backward)) return 0;
    if (!backward) return route_forward(a, *shape, LSN_NHWC).prepared ? 1 : 0;
    return route_backward(a, *shape, LSN_NHWC, shape->gather_workspace, gather_ws_bytes(*shape), false).prepared ? 1 : 0;
}

// (backward: the answer is for a call that asks for grad_weight)
int lsn_dcn_pitched_ok(const lsn_dcn_shape *shape, int n_levels, const lsn_dcn_level *levels, int backward)
{
    using namespace lsn;
    DcnArgs a;
    if (!query_args(a, shape, n_levels, levels, backward)) return 0;
    if (!backward) return route_forward(a, *shape, LSN_NHWC).pitched ? 1 : 0;
    return route_backward(a, *shape, LSN_NHWC, shape->gather_workspace, gather_ws_bytes(*shape), true).pitched ? 1 : 0;
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
    for (int i = 0; i < n_levels; ++i) {
        LSN_CHECK(levels[i].input && levels[i].grad_output, "level %d: input/grad_output is NULL", i);
        a.lv[i].x = levels[i].input;
        a.lv[i].gout = levels[i].grad_output;
        a.lv[i].gx = levels[i].grad_input;
    }
    void *gws = s.gather_workspace;
    DcnRoute r = route_backward(a, s, layout, gws, gather_ws_bytes(s), false);
    if (!r.gather()) return fail(LSN_ERR_UNSUPPORTED, "lsn_dcn_anchor_lists: this call builds no anchor lists (route without the gather pass)");
    const GatherPlan &pl = r.plan;
    counts[0] = pl.nsamples, counts[1] = pl.nanchors;
    if (!sample_anchor && !list_start && !list_sample) return 0;   // the sizes only
    LSN_CHECK(sample_anchor && list_start && list_sample, "lsn_dcn_anchor_lists: all three outputs or none");
    unsigned char *w = reinterpret_cast<unsigned char *>(gws);
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
