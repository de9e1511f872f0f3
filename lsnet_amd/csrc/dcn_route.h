// The route of a deformable-convolution call -- which kernel serves each pass and what else that fixes -- and the workspace plan of
// the atomic-free gather pass: functions of the call's shape, plain C++ without HIP, library state or device pointers, so that
// tools/dcn_route_cases.cpp (tests/test_dcn_route_host.py) compiles them on the host.  dcn.hip fills the shape once per call
// (route_shape: the only place that turns pointers, debug bits and the math mode into facts), decides here before anything is
// launched and hands the DcnRoute to its launchers, which do not ask again.  The three queries of the C ABI
// (lsn_dcn_backward_workspace_bytes, lsn_dcn_prepared_ok, lsn_dcn_pitched_ok) read the same answers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dcn_sort_plan.h"

// the kernels' own values (dcn.hip checks each against the kernel headers)
constexpr int DR_MAXLV = 16;                             // MAXLV
constexpr int DR_GT = 4;                                 // GT: block edge of the gather's pixel blocks
constexpr int DR_GF_CH = 64, DR_GC_COLS = 64;            // GF_CH, GC_COLS: channels per workgroup of the grouped forward / column gradients
constexpr int DR_WG_BP = 32, DR_WG_BN = 64, DR_WG_BM = 256;   // WG_BP, WG_BN, WG_BM: tile of the split weight-gradient kernels
constexpr size_t DR_TAP_BYTES = 32, DR_GENTRY_BYTES = 16;   // sizeof(Tap), sizeof(GEntry)
constexpr size_t DR_LDS_MAX = 160 * 1024;                 // LDS a workgroup can have (gfx950)
constexpr int DR_FP32_BM = 64;                            // BWD_BM, and BM of every dcn_fwd_kernel: pixels per workgroup of the fp32 kernels

struct DcnRouteLevel {
    int B, H, W, Ho, Wo;
    int P;                    // B * Ho * Wo
    bool gx, goff, gmsk;      // grad_input / grad_offset / grad_mask are asked for
    bool x_aligned16, gout_aligned16;
    int gx_id;                // levels with the same id share one grad_input buffer: the index of the first level with that buffer
};

struct DcnRouteShape {
    int n;   // levels
    DcnRouteLevel lv[DR_MAXLV];
    int C, Co, kh, kw, groups, dg;
    int SL;                  // channel segment length = min(C / groups, C / dg)
    int opitch;              // floats per pixel of out / grad_output (>= Co)
    int np, npl;             // bf16 products per product of the math mode (0: exact, 1, 3, 6) and its planes per operand
    bool nchw;               // a reference-layout (LSN_NCHW) entry point: neither out_pitch nor a prepared image, own gather scratch
    bool want_wgrad;         // backward: grad_weight is asked for (the queries say which case they answer for)
    bool workspace;          // the caller's weight workspace is there
    bool gather_ws;          // the caller's gather workspace is there, ...
    size_t gather_ws_bytes;  // ... this large, ...
    bool gather_ws_aligned16;   // ... and 16-byte aligned
    bool general_gemms;      // LSN_DBG_GENERAL_GEMMS: the kernels of dcn_kernels.h only -- tests, A/B runs
    bool atomic_scatter;     // LSN_DBG_ATOMIC_SCATTER: the atomic scatter kernels -- tests
    bool anchor_one_wave;    // LSN_DBG_ANCHOR_ONE_WAVE
    // what the kernels say of themselves for this shape and math mode (dcn.hip asks their own functions)
    size_t fwd_mm_lds, xn_lds, bwd_xn_lds, fwd_grouped_lds;   // dcn_fwd_mm_lds_bytes, xn_lds_bytes, bwd_xn_lds_bytes, dcn_fwd_grouped_lds_bytes
    size_t wfrag_fwd, wfrag_bwd;   // cv_wfrag_bytes of the forward (Co, K, C) image and of the backward's transposed 1x1 view (K C, 1, Co)
};

constexpr int dr_cdiv(int a, int b) { return (a + b - 1) / b; }
// 32-bit offsets: `elems` elements of `bytes_per` bytes stay below 2^31 (bytes_per = 1: a bound on the element count)
inline bool fits_i32(int64_t elems, int bytes_per = 1) { return elems * bytes_per < ((int64_t)1 << 31); }
inline int64_t in_elems(const DcnRouteShape &s, int i) { return (int64_t)s.lv[i].B * s.lv[i].H * s.lv[i].W * s.C; }
inline int64_t col_elems(const DcnRouteShape &s, int i) { return (int64_t)s.lv[i].P * s.kh * s.kw * s.C; }   // column-gradient rows

// VEC kernels need 16-byte aligned float4 rows: channel counts that are multiples of 4
inline bool vec_ok(const DcnRouteShape &s)
{
    const int Cg = s.C / s.groups, Cog = s.Co / s.groups;
    return (Cg % 4 == 0) && (Cog % 4 == 0) && (s.Co % 4 == 0) && (s.SL % 4 == 0);
}

// ---- the kernels of dcn_mm_kernels.h (dense-convolution skeleton): conditions ----
inline bool mm_common_ok(const DcnRouteShape &s)
{
    if (s.np == 0 || s.groups != 1 || s.dg < 1 || s.C % s.dg != 0 || s.general_gemms) return false;
    for (int i = 0; i < s.n; ++i)   // 32-bit buffer offsets
        if (!fits_i32(in_elems(s, i), 4) || !fits_i32((int64_t)s.lv[i].P * s.opitch, 4)) return false;
    return true;
}

inline bool mm_fwd_ok(const DcnRouteShape &s)
{
    if (!mm_common_ok(s) || (s.C / s.dg) % 32 != 0 || s.Co % 128 != 0) return false;
    if (s.fwd_mm_lds > 80 * 1024) return false;
    return fits_i32((int64_t)s.wfrag_fwd);
}

// backward-data GEMM as a 1x1 convolution (conv.hip conv_mm_rows) + corner sums in the gather pass: every level that
// wants offset / mask gradients must also want grad_input (its samples are then on the anchor lists); the fragment image
// has to fit the caller's weight workspace (8 bytes per weight element, include/lsnet_hip.h)
inline bool mm_bwd_ok(const DcnRouteShape &s)
{
    if (!mm_common_ok(s) || s.C % 4 != 0 || s.Co % 4 != 0) return false;
    for (int i = 0; i < s.n; ++i)
        if ((s.lv[i].goff || s.lv[i].gmsk) && !s.lv[i].gx) return false;
    return fits_i32((int64_t)s.wfrag_bwd) && s.wfrag_bwd <= (size_t)8 * s.Co * s.kh * s.kw * s.C;
}

// the split one-workgroup-per-CU kernel (dcn_fwd_xn_kernel) needs float4 rows and 32-bit byte offsets into x and w
inline bool xn_ok(const DcnRouteShape &s)
{
    if (s.Co / s.groups <= 64 || !vec_ok(s)) return false;
    if (!fits_i32((int64_t)s.Co * s.kh * s.kw * (s.C / s.groups), 4)) return false;
    for (int i = 0; i < s.n; ++i)
        if (!fits_i32(in_elems(s, i), 4)) return false;
    return true;
}

// ---- the fp32 kernels of dcn_kernels.h (dcn_fwd_kernel, dcn_bwd_data_kernel): the last kernel of their pass, with the tap table
// [64 pixels][KD = kh kw dg] of a workgroup in LDS like every kernel in front of them.  Their LDS need is part of the route: a
// call whose table no tile of theirs leaves room for is refused before anything is launched (DcnRoute::lds_over). ----
// dcn_fwd_kernel<64, BN>: As[64][33] + Bs[BN][33] floats, tab[64][KD]
constexpr size_t fwd_fp32_lds(int BN, int KD) { return (size_t)(DR_FP32_BM + BN) * 33 * 4 + (size_t)DR_FP32_BM * KD * DR_TAP_BYTES; }
// dcn_bwd_data_kernel<RED>: Bs[RED][32] floats, tab[64][KD], gacc[64][KD][3] floats
constexpr size_t bwd_fp32_lds(int RED, int KD) { return (size_t)RED * 32 * 4 + (size_t)DR_FP32_BM * KD * (DR_TAP_BYTES + 12); }
// The wide tile (256 output channels of a group per workgroup / per reduction slab) where a group has more than 64 and the
// table leaves room, else the 64-wide one: more column blocks (forward) or reduction slabs (backward), the same sums.
inline int fwd_fp32_bn(const DcnRouteShape &s)
{
    return s.Co / s.groups > 64 && fwd_fp32_lds(256, s.kh * s.kw * s.dg) <= DR_LDS_MAX ? 256 : 64;
}
inline int bwd_fp32_red(const DcnRouteShape &s)
{
    return s.Co / s.groups > 64 && bwd_fp32_lds(256, s.kh * s.kw * s.dg) <= DR_LDS_MAX ? 256 : 64;
}

// ---- grouped calls (dcn_grouped_kernels.h): ResNeXt's 64 groups of 8 / 16 / 32 channels ----
inline bool grouped_inputs_ok(const DcnRouteShape &s)   // 16-byte loads at 32-bit element offsets
{
    for (int i = 0; i < s.n; ++i)
        if (!fits_i32(in_elems(s, i)) || !s.lv[i].x_aligned16) return false;
    return true;
}

inline bool grouped_fwd_ok(const DcnRouteShape &s)
{
    if (s.groups <= 1 || s.C % s.groups != 0 || s.Co != s.C) return false;
    const int cg = s.C / s.groups;
    if (!(cg == 8 || cg == 16 || cg == 32) || s.C % DR_GF_CH != 0 || s.C % s.dg != 0 || (s.C / s.dg) % DR_GF_CH != 0) return false;
    return s.fwd_grouped_lds <= 64 * 1024 && grouped_inputs_ok(s);
}

// 32-bit buffer offsets into the input and into every level's column-gradient rows (backward-data, every kernel in front
// of the gather pass)
inline bool bwd_offsets_ok(const DcnRouteShape &s)
{
    for (int i = 0; i < s.n; ++i)
        if (!fits_i32(in_elems(s, i), 4) || !fits_i32(col_elems(s, i), 4)) return false;
    return true;
}

// round 2's split GEMM (dcn_bwd_data_xn_kernel) on the transposed weight planes the caller's `workspace` holds
inline bool bwd_x3_ok(const DcnRouteShape &s)
{
    if (s.np == 0 || s.groups != 1) return false;
    if (s.Co > 256 || s.Co % 8 != 0 || s.C % 4 != 0) return false;
    if (!fits_i32((int64_t)s.kh * s.kw * s.C * s.Co, 6)) return false;
    if (s.bwd_xn_lds > 80 * 1024) return false;
    return bwd_offsets_ok(s);
}

// Exact-fp32 column gradients (dcn_gcol_grouped_kernel: fmaf chains per group) in front of the gather pass: grouped calls
// (config 4: 64 groups) in every math mode, and -- round 6 -- EVERY call of LSN_MATH_FP32: the exact mode used to scatter
// with fp32 atomics (round 1's kernels) and was the less reproducible, less exact of the modes; it now
// shares the atomic-free, bit-reproducible gather with the default mode and differs from it in the GEMM arithmetic only.
// Levels that want offset / mask gradients must want grad_input (anchor lists).
inline bool bwd_grouped_ok(const DcnRouteShape &s)
{
    if (s.groups <= 1 && s.np != 0) return false;
    if (s.C % s.groups != 0 || s.Co % s.groups != 0 || (s.C / s.groups) % 4 != 0 || s.C % s.dg != 0) return false;
    if ((s.C / s.dg) % 4 != 0 || s.atomic_scatter) return false;
    for (int i = 0; i < s.n; ++i)
        if ((s.lv[i].goff || s.lv[i].gmsk) && !s.lv[i].gx) return false;
    return bwd_offsets_ok(s);
}

// ---- atomic-free grad_input: workspace plan of the list sort / gather sequence (dcn_gather_kernels.h) ----
// a grad_input buffer with the levels that scatter into it: `level` owns it (the first of them; dcn.hip takes the pointers there)
struct GatherPlanGroup {
    int level;
    int B, H, W;
    int abase;   // first anchor id: anchors (B, H+1, W+1), (y0+1, x0+1) row-major
    int first;   // block walk: first 4x4 pixel block (blk0); anchor path: first anchor in the S buffer (a0)
};

struct GatherPlan {
    bool ok = false;
    int nsamples = 0, nanchors = 0;
    size_t o_gcol = 0, o_hist = 0, o_start = 0, o_key = 0, o_ent = 0, o_gtap = 0, bytes = 0;
    size_t o_S = 0, o_H = 0, o_pairs = 0;
    int prow0[DR_MAXLV] = {}, abase[DR_MAXLV] = {};   // of every level: first pixel row, first anchor of its grad_input buffer
    GatherPlanGroup blk[DR_MAXLV] = {};   // groups gathered per 4x4 pixel block
    int nblk = 0, NB = 0;                 // ... and the blocks of all of them
    GatherPlanGroup anc[DR_MAXLV] = {};   // groups with long lists: gathered per anchor (dcn_anchor_sum / combine)
    int nanc = 0, NA = 0;                 // ... and the anchors of all of them
    int ncb = 1;                 // 256-channel blocks the per-anchor sums split over blockIdx.y (AnchorArgs::ncb)
    long long hb_slot = 0;       // floats between the corner-sum slots of two channel blocks
    int anchor_pixels = 0;
    int na_long = 0;             // the first na_long anchors of the S buffer belong to long-list groups (4 waves each)
    int64_t block_samples = 0;   // samples (upper bound) of the block-gathered groups
};

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// gx_id: levels with the same grad_input share an anchor grid.
// all_anchor: every group on the per-anchor path (route_backward says when).
inline GatherPlan gather_plan(const DcnRouteShape &s, bool all_anchor)
{
    GatherPlan pl;
    const int K = s.kh * s.kw, KD = K * s.dg;
    int64_t prow = 0, anchors = 0, Q = 0;
    GatherPlanGroup grp[DR_MAXLV];
    int ng = 0;
    int64_t gsamp[DR_MAXLV] = {};   // samples (upper bound: every tap valid) that scatter into each group
    for (int i = 0; i < s.n; ++i) {
        const DcnRouteLevel &L = s.lv[i];
        pl.prow0[i] = (int)prow;
        prow += L.P;
        if (!L.gx) continue;
        int gi = -1;
        for (int j = 0; j < ng; ++j)
            if (grp[j].level == L.gx_id) gi = j;
        if (gi < 0) {
            gi = ng++;
            grp[gi] = GatherPlanGroup{i, L.B, L.H, L.W, (int)anchors, (int)Q};
            anchors += (int64_t)L.B * (L.H + 1) * (L.W + 1);
            Q += (int64_t)L.B * dr_cdiv(L.H, DR_GT) * dr_cdiv(L.W, DR_GT);
        } else if (grp[gi].B != L.B || grp[gi].H != L.H || grp[gi].W != L.W) {
            return pl;   // one buffer, two shapes: not a valid call for this path
        }
        pl.abase[i] = grp[gi].abase;
        gsamp[gi] += (int64_t)L.P * KD;
    }
    if (ng == 0) return pl;
    if (prow * KD >= ((int64_t)1 << 30) || anchors >= ((int64_t)1 << 30) || Q >= ((int64_t)1 << 30)) return pl;
    if (s.C % 4 != 0 || (s.C / s.dg) % 4 != 0) return pl;
    pl.nsamples = (int)(prow * KD);
    pl.nanchors = (int)anchors;
    if (ds_digit_bits(pl.nanchors) > DS_MAX_DIGIT_BITS) return pl;   // (cannot happen below 2^30 anchors: the LDS of the list sort)
    // Groups with more than ~400 samples per 4x4 pixel block go to the per-anchor gather (the pyramid op's coarse source
    // levels); the others keep the block walk.
    constexpr int anchor_thr = 400;
    {
        // anchor path: every group when the unweighted-GEMM pipeline can serve the call (its corner sums are cheapest per
        // anchor), otherwise the groups above the threshold.  Long-list groups first: they get four waves per anchor.
        bool to_anchor[DR_MAXLV], is_long[DR_MAXLV];
        int64_t q = 0;
        for (int j = 0; j < ng; ++j) {
            const GatherPlanGroup &G = grp[j];
            const int64_t nblk = (int64_t)G.B * dr_cdiv(G.H, DR_GT) * dr_cdiv(G.W, DR_GT);
            const int64_t nanch = (int64_t)G.B * (G.H + 1) * (G.W + 1);
            to_anchor[j] = all_anchor || (anchor_thr > 0 && gsamp[j] > (int64_t)anchor_thr * nblk);
            constexpr int long_thr = 40;
            is_long[j] = !all_anchor || gsamp[j] > (int64_t)long_thr * nanch;   // mean list length (upper bound)
        }
        for (int pass = 0; pass < 2; ++pass) {
            for (int j = 0; j < ng; ++j) {
                const GatherPlanGroup &G = grp[j];
                if (!to_anchor[j] || is_long[j] != (pass == 0)) continue;
                pl.anc[pl.nanc] = G, pl.anc[pl.nanc++].first = pl.NA;
                pl.NA += G.B * (G.H + 1) * (G.W + 1);
                pl.anchor_pixels += G.B * G.H * G.W;
            }
            if (pass == 0) pl.na_long = pl.NA;
        }
        for (int j = 0; j < ng; ++j) {
            if (to_anchor[j]) continue;
            const GatherPlanGroup &G = grp[j];
            pl.blk[pl.nblk] = G, pl.blk[pl.nblk++].first = (int)q;
            q += (int64_t)G.B * dr_cdiv(G.H, DR_GT) * dr_cdiv(G.W, DR_GT);
            pl.block_samples += gsamp[j];
        }
        Q = q;
    }
    pl.NB = (int)Q;
    size_t o = 0;
    pl.o_gcol = o, o = align256(o + (size_t)prow * K * s.C * sizeof(float));
    // the histogram of one pass, [digit][block] + the digits' totals: (blocks + 1) x 2^db ints with 2^db <= 2 sqrt(anchors),
    // i.e. at most 4 bytes per sample + 16 sqrt(anchors) -- less than the anchor counters and sample ranks it replaces
    pl.o_hist = o, o = align256(o + ds_hist_ints(pl.nsamples, pl.nanchors) * sizeof(int));
    pl.o_start = o, o = align256(o + ((size_t)pl.nanchors + 1) * sizeof(int));
    pl.o_key = o, o = align256(o + (size_t)pl.nsamples * sizeof(int));
    pl.o_ent = o, o = align256(o + (size_t)pl.nsamples * DR_GENTRY_BYTES);
    pl.o_gtap = o, o = align256(o + ((size_t)pl.nsamples + 1) * DR_TAP_BYTES);   // + the all-zero entry
    pl.o_S = o, o = align256(o + (size_t)pl.NA * 4 * s.C * sizeof(float));
    // corner sums (dcn_offgrad_kernel): one slot per 256-channel block where the per-anchor sums split them over blockIdx.y
    // (every group on the per-anchor path, C > 256; dcn_gather_kernels.h AnchorArgs::ncb)
    // (LSN_DBG_ANCHOR_ONE_WAVE: one wave walks all blocks of its anchor, the form until round 6 -- tests; the workspace is sized for
    // the split either way, so a size asked for under one setting serves a launch under the other)
    const int ncb_max = (pl.NB == 0 && pl.nanc > 0 && s.C > 256) ? dr_cdiv(s.C, 256) : 1;
    pl.ncb = s.anchor_one_wave ? 1 : ncb_max;
    pl.hb_slot = (long long)pl.nsamples * 4;
    pl.o_H = o, o = align256(o + (size_t)pl.nsamples * 4 * sizeof(float) * ncb_max);
    pl.o_pairs = o, o = align256(o + (size_t)pl.nsamples * 2 * 2 * sizeof(int));   // the (key, sample) pairs of the sort, ping and pong
    pl.bytes = o;
    pl.ok = true;
    return pl;
}

// Pixel splits of a weight-gradient launch: the grid (columns x splits x co blocks) fills ONE round of the blocks the chip
// holds at once (256 CUs x per_cu), rounded DOWN.  Measured on the benchmark step (profiles/r2_wgrad_rounds.txt): the
// old cdiv(1024, 36) = 29 splits made 1044 blocks = two full rounds plus a third with 20 blocks (0.88 ms per DCN
// launch); 28 splits 0.68 ms; one round instead of two is the same for the DCN launches and 1.1 ms / step faster over
// the dense layers (half the fp32 atomics of the epilogues).
inline int wgrad_splits(int cols, int per_cu)
{
    const int slots = 256 * per_cu;
    int s = slots / cols;
    return s < 1 ? 1 : s;
}

// weight gradient on the kernels of dcn_mm_kernels.h (it also needs the tap table of the gather pass: route_backward)
inline bool mm_wgrad_ok(const DcnRouteShape &s) { return mm_common_ok(s) && s.Co % 256 == 0 && (s.C / s.dg) % 64 == 0; }
// ... and its fragment-order image of grad_output (nchunks 32-pixel chunks) at 32-bit byte offsets
inline bool wgrad_mm_image_ok(const DcnRouteShape &s, int nchunks) { return fits_i32((int64_t)nchunks * 2 * (s.Co / 32) * s.npl, 1024); }

inline bool grouped_wgrad_ok(const DcnRouteShape &s)
{
    if (s.groups <= 1 || s.C % s.groups != 0 || s.Co != s.C || s.kh * s.kw > 9) return false;
    const int cg = s.C / s.groups;
    if (!(cg == 4 || cg == 8 || cg == 16 || cg == 32) || ((int64_t)s.C * cg) % 256 != 0 || s.C % s.dg != 0) return false;
    const int nch = cg >= 16 ? cg : 256 / cg;
    if ((s.C / s.dg) % nch != 0 || s.C % nch != 0) return false;
    return grouped_inputs_ok(s);
}

// ---- the route of a call: which kernel serves each pass and what else that fixes.  route_forward / route_backward decide
// it once, before anything is launched; they are the only callers of the *_ok predicates and of gather_plan. ----
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
    bool vec = false;        // float4 rows (vec_ok): the VEC forms of the fp32 kernels
    bool pitched = false;    // out_pitch != Co is served (lsn_dcn_pitched_ok)
    bool prepared = false;   // weights_prepared is served (lsn_dcn_prepared_ok)
    int gcol_ks = 0;         // GATHER_GROUPED: k-steps of dcn_gcol_mfma_kernel; 0: the fmaf chains of dcn_gcol_grouped_kernel
    int wg_steps = 0;        // weight gradient: 32-pixel steps of all levels
    int wg_ncol = 0, wg_nz = 0, wg_splits = 0;   // WG_XN_* / WG_FP32_*: grid of the split kernels (columns, co blocks, pixel splits)
    bool own_gather_ws = false;        // LSN_NCHW without the caller's gather workspace: plan.bytes of the call's own scratch
    int fp32_bn = 0;         // FWD_FP32: output channels per workgroup of dcn_fwd_kernel (256 or 64)
    int fp32_red = 0;        // SCATTER_FP32: output channels per reduction slab of dcn_bwd_data_kernel (256 or 64)
    size_t lds_over = 0;     // != 0: no kernel serves the pass -- the LDS bytes (> DR_LDS_MAX) the fp32 kernel would need: the call is refused
    GatherPlan plan;                   // GATHER_*: computed here, once
    bool gather() const { return data == GATHER_GROUPED || data == GATHER_MM || data == GATHER_XN; }
};

// Order: mm -> grouped -> xn -> fp32 (refused where its tap table does not fit: lds_over).  The reference-layout (LSN_NCHW)
// entry points take the same kernels but neither out_pitch nor a prepared image.
inline DcnRoute route_forward(const DcnRouteShape &s)
{
    DcnRoute r;
    r.vec = vec_ok(s);
    if (s.workspace && mm_fwd_ok(s)) {
        r.fwd = FWD_MM, r.image = IMG_FRAGMENT;
    } else if (grouped_fwd_ok(s)) {
        r.fwd = FWD_GROUPED;
    } else if (s.np != 0 && xn_ok(s) && s.xn_lds <= 160 * 1024) {
        r.fwd = FWD_XN;   // with a workspace the weights are split once instead of in every block
        if (s.workspace && (s.C / s.groups) % 8 == 0) r.fwd = FWD_XN_PLANES, r.image = IMG_PLANES;
    }
    if (r.fwd == FWD_FP32) {
        r.fp32_bn = fwd_fp32_bn(s);
        const size_t lds = fwd_fp32_lds(r.fp32_bn, s.kh * s.kw * s.dg);
        if (lds > DR_LDS_MAX) r.lds_over = lds;
    }
    r.pitched = r.prepared = !s.nchw && r.fwd == FWD_MM;
    return r;
}

// k-steps of the fp32-MFMA column gradients (dcn_grouped_kernels.h dcn_gcol_mfma_kernel); 0: the fmaf-chain kernel
inline int gcol_mfma_ksteps(const DcnRouteShape &s)
{
    const int Cg = s.C / s.groups, Cog = s.Co / s.groups;
    if (s.C % DR_GC_COLS != 0 || s.opitch % 4 != 0) return 0;
    for (int i = 0; i < s.n; ++i)
        if (!s.lv[i].gout_aligned16) return 0;
    if (s.groups == 1) return (s.Co == 64 || s.Co == 128 || s.Co == 256) ? s.Co / 4 : 0;
    return (Cog == Cg && (Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32)) ? (Cg == 32 ? 8 : 4) : 0;
}

// grid of the split weight-gradient kernels (dcn_wgrad_kernel / dcn_wgrad_xn_kernel): columns, co blocks; returns the pixel splits
inline int wgrad_split_grid(const DcnRouteShape &s, int nsteps, int *ncol, int *nz)
{
    const int K = s.kh * s.kw, Cg = s.C / s.groups, Cog = s.Co / s.groups;
    *ncol = s.groups * K * (Cg / s.SL) * dr_cdiv(s.SL, DR_WG_BN), *nz = dr_cdiv(Cog, DR_WG_BM);
    int n = wgrad_splits(*ncol * *nz, 2);   // 2 resident blocks per CU (246 VGPRs, 78 KB LDS)
    if (n > nsteps) n = nsteps;
    if (n < 1) n = 1;
    return n > 65535 ? 65535 : n;
}

// Backward-data: the gather path where a column-gradient kernel serves the call -- grouped (groups > 1, or any call of
// LSN_MATH_FP32), else mm, else xn -- and a gather workspace holds the plan; else scatter xn; else the fp32 scatter (refused
// where its tap table does not fit: lds_over).
// Weight gradient: grouped (dense grad_output, 4 | weight elements) -> mm (reads the gather pass's tap table) -> the split
// kernels.  A prepared image is served by GATHER_MM (so: groups = 1, a split-bf16 mode, even Co, some data gradient), out_pitch
// by GATHER_MM and -- when grad_weight is asked for -- WG_MM; neither by the reference-layout (LSN_NCHW) entry points, which
// get the call's own gather scratch instead of the caller's.
inline DcnRoute route_backward(const DcnRouteShape &s)
{
    DcnRoute r;
    r.vec = vec_ok(s);
    const int K = s.kh * s.kw;
    bool any_data = false;
    for (int i = 0; i < s.n; ++i) any_data = any_data || s.lv[i].gx || s.lv[i].goff || s.lv[i].gmsk;
    if (any_data) {
        // can_split: `workspace` gets a bf16 image of the weights (8 bytes per weight element: even Co for the planes)
        const bool can_split = s.workspace && s.np && s.groups == 1 && s.Co % 2 == 0;
        const bool grouped = bwd_grouped_ok(s), mm = mm_bwd_ok(s), x3 = can_split && bwd_x3_ok(s);
        const DataKernel cand = s.atomic_scatter                          ? DATA_NONE
                                : grouped                                 ? GATHER_GROUPED
                                : (can_split && mm && bwd_offsets_ok(s)) ? GATHER_MM
                                : x3                                      ? GATHER_XN
                                                                          : DATA_NONE;
        bool fits = false;
        if (cand != DATA_NONE && (s.gather_ws || s.nchw)) {
            // (all_anchor keys on what the arguments admit, not on the kernel taken: the workspace size a caller asked for
            // without `workspace` serves the call with it)
            r.plan = gather_plan(s, mm || grouped);
            r.own_gather_ws = !s.gather_ws && r.plan.ok;
            fits = r.plan.ok && (r.own_gather_ws || r.plan.bytes <= s.gather_ws_bytes);
        }
        r.data = fits ? cand : x3 ? SCATTER_XN : SCATTER_FP32;
        if (r.data == GATHER_GROUPED) r.gcol_ks = gcol_mfma_ksteps(s);
        if (r.data == SCATTER_FP32) {
            r.fp32_red = bwd_fp32_red(s);
            const size_t lds = bwd_fp32_lds(r.fp32_red, K * s.dg);
            if (lds > DR_LDS_MAX) r.lds_over = lds;
        }
        // (the transposed planes are written for every call that can split, also where the fp32 scatter then ignores them)
        r.image = r.data == GATHER_MM ? IMG_FRAGMENT : can_split ? IMG_PLANES_T : IMG_NONE;
        r.prepared = !s.nchw && r.data == GATHER_MM;
    }
    if (s.want_wgrad) {
        int64_t rows = 0, steps = 0;
        for (int i = 0; i < s.n; ++i) rows += s.lv[i].P, steps += dr_cdiv(s.lv[i].P, DR_WG_BP);
        r.wg_steps = (int)steps;
        const size_t nW = (size_t)s.Co * K * (s.C / s.groups);
        // the tap table of the gather pass, 16-byte aligned (the call's own scratch is)
        const bool tap_table = r.gather() && (r.own_gather_ws || s.gather_ws_aligned16);
        if (grouped_wgrad_ok(s) && s.opitch == s.Co && nW % 4 == 0 && rows < ((int64_t)1 << 30)) {
            r.wgrad = WG_GROUPED;
        } else if (mm_wgrad_ok(s) && tap_table && wgrad_mm_image_ok(s, r.wg_steps)) {
            r.wgrad = WG_MM;
        } else {
            // one partial gradient per pixel split + an ordered reduce instead of fp32 atomics (deterministic) where they fit
            r.wg_splits = wgrad_split_grid(s, r.wg_steps, &r.wg_ncol, &r.wg_nz);
            const bool ordered = nW % 4 == 0 && (size_t)r.wg_splits * (nW + s.Co) * sizeof(float) <= ((size_t)256 << 20);
            r.wgrad = s.np ? (ordered ? WG_XN_ORDERED : WG_XN_ATOMIC) : (ordered ? WG_FP32_ORDERED : WG_FP32_ATOMIC);
        }
    }
    r.pitched = !s.nchw && r.data == GATHER_MM && (!s.want_wgrad || r.wgrad == WG_MM);
    return r;
}
