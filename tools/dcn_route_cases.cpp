// The route of a deformable-convolution call and the workspace plan of its gather pass (lsnet_amd/csrc/dcn_route.h) on the host,
// without a GPU: one line per case, "<name>: <forward kernel>/<image> <data kernel>/<image> <weight-gradient kernel> ok" or
// "... MISMATCH" with the route and plan it got and the ones it expected, and a non-zero exit status when a case misses its row.
// tests/test_dcn_route_host.py builds this with g++ under the address and undefined-behaviour sanitizers.
//
// A row is a shape as dcn.hip's route_shape fills it, and the whole answer as text: the forward route, the backward route with
// the carried weight-gradient grid (columns/co blocks/splits), and the plan -- samples, anchors, the offsets o_gcol, o_hist,
// o_start, o_key, o_ent, o_gtap, o_S, o_H, o_pairs, bytes, the group counts, per level prow0:abase, per block-walk group
// level:B,H,W,abase,blk0 and per anchor group level:B,H,W,abase,a0.  The expected texts were printed by the functions this header
// replaced (csrc/dcn.hip's route_forward / route_backward / gather_plan of the commit before it), called through the C ABI's
// argument filling for the same call; so were the numbers of kernels(): what the kernels' own functions give for the row's taps,
// channels and math mode (dcn_fwd_mm_lds_bytes, xn_lds_bytes, bwd_xn_lds_bytes, dcn_fwd_grouped_lds_bytes, cv_wfrag_bytes
// forward and backward).  Rows at a cap take the shape whose real numbers lie on either side of it.  The rows "kd N" cut each LDS
// threshold in KD = kh kw dg at the largest count the kernel keeps and at the next one; their numbers follow from the formulas
// quoted above each pair, and their texts also state the fp32 kernels' part of the route (" | fp32 bn red over=fwd/bwd").
// Unless a case says otherwise: six products per product, one level of 2 x 13 x 17 pixels that wants all three data gradients,
// both workspaces (the gather workspace large enough), aligned pointers, the debug bits clear, channels-last, no grad_weight.
//
// Guards no call reaches on its own, because the guards in front of them are stricter:
//  * gather_plan's prow * KD >= 2^30: every gather route sits behind bwd_offsets_ok, P * K * C * 4 < 2^31 per level, i.e.
//    P * K * C < 2^29, and dg <= C / 4 (4 | C / dg), so P * K * dg < 2^27 per level and < 2^31 over sixteen levels only with
//    more than eight levels at that bound -- each with an input of its own below 2^29 elements; the last row calls gather_plan
//    directly instead.  anchors / blocks >= 2^30 and the digit-width check behind them fall to the same bound on the inputs.
//  * gcol_mfma_ksteps' opitch % 4 != 0: out_pitch is 0 or a multiple of 4, so the pitch is odd only as Co itself, and such a
//    Co is none of 64 / 128 / 256 (nor equal to a C that 64 divides): the row "pitch 66" passes through the guard, but the
//    lines behind it would answer 0 as well.
//  * WG_GROUPED's rows < 2^30: needs 2^30 output pixels in one call; no row.
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <string>

#include "dcn_route.h"

static const char *FWD[] = {"FWD_MM", "FWD_GROUPED", "FWD_XN_PLANES", "FWD_XN", "FWD_FP32"};
static const char *DATA[] = {"DATA_NONE", "GATHER_GROUPED", "GATHER_MM", "GATHER_XN", "SCATTER_XN", "SCATTER_FP32"};
static const char *WG[] = {"WG_NONE", "WG_GROUPED", "WG_MM", "WG_XN_ORDERED", "WG_XN_ATOMIC", "WG_FP32_ORDERED", "WG_FP32_ATOMIC"};
static const char *IMG[] = {"IMG_NONE", "IMG_FRAGMENT", "IMG_PLANES", "IMG_PLANES_T"};

struct Lv {
    int B, H, W, Ho, Wo;
    int gx;   // the first level with the same grad_input; -1: none
    bool goff, gmsk;
};
static const Lv L0 = {2, 13, 17, 13, 17, 0, true, true};

static DcnRouteShape shape(int C, int Co, int kh, int kw, int groups, int dg, std::initializer_list<Lv> levels)
{
    DcnRouteShape s = {};
    for (const Lv &v : levels) {
        DcnRouteLevel &L = s.lv[s.n++];
        L.B = v.B, L.H = v.H, L.W = v.W, L.Ho = v.Ho, L.Wo = v.Wo, L.P = v.B * v.Ho * v.Wo;
        L.gx = v.gx >= 0, L.goff = v.goff, L.gmsk = v.gmsk;
        L.x_aligned16 = L.gout_aligned16 = true;
        L.gx_id = v.gx >= 0 ? v.gx : 0;   // (levels without grad_input share "none": what comparing their NULL pointers gives)
    }
    s.C = C, s.Co = Co, s.kh = kh, s.kw = kw, s.groups = groups, s.dg = dg;
    s.SL = C / groups < C / dg ? C / groups : C / dg;
    s.opitch = Co;
    s.workspace = s.gather_ws = s.gather_ws_aligned16 = true;
    s.gather_ws_bytes = (size_t)1 << 40;
    return s;
}

static void kernels(DcnRouteShape &s, int np, int npl, size_t fwd_mm_lds, size_t xn_lds, size_t bwd_xn_lds, size_t fwd_grouped_lds,
                    size_t wfrag_fwd, size_t wfrag_bwd)
{
    s.np = np, s.npl = npl;
    s.fwd_mm_lds = fwd_mm_lds, s.xn_lds = xn_lds, s.bwd_xn_lds = bwd_xn_lds, s.fwd_grouped_lds = fwd_grouped_lds;
    s.wfrag_fwd = wfrag_fwd, s.wfrag_bwd = wfrag_bwd;
}

static void misalign_gout(DcnRouteShape &s)
{
    for (int i = 0; i < s.n; ++i) s.lv[i].gout_aligned16 = false;
}

static std::string text(const DcnRouteShape &s, const DcnRoute &f, const DcnRoute &r)
{
    char b[256];
    std::string o;
    snprintf(b, sizeof b, "fwd=%d image=%d pitched=%d prepared=%d vec=%d", (int)f.fwd, (int)f.image, (int)f.pitched, (int)f.prepared, (int)f.vec);
    o += b;
    snprintf(b, sizeof b, " | data=%d image=%d prepared=%d pitched=%d gcol_ks=%d own=%d wgrad=%d wg_steps=%d grid=%d/%d/%d", (int)r.data,
             (int)r.image, (int)r.prepared, (int)r.pitched, r.gcol_ks, (int)r.own_gather_ws, (int)r.wgrad, r.wg_steps, r.wg_ncol, r.wg_nz, r.wg_splits);
    o += b;
    const GatherPlan &pl = r.plan;
    snprintf(b, sizeof b, " | plan ok=%d", (int)pl.ok);
    o += b;
    if (!pl.ok) return o;
    snprintf(b, sizeof b, " ns=%d na=%d o=%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu bytes=%zu", pl.nsamples, pl.nanchors, pl.o_gcol, pl.o_hist, pl.o_start,
             pl.o_key, pl.o_ent, pl.o_gtap, pl.o_S, pl.o_H, pl.o_pairs, pl.bytes);
    o += b;
    snprintf(b, sizeof b, " NB=%d NA=%d na_long=%d ncb=%d hb_slot=%lld apx=%d bs=%lld", pl.NB, pl.NA, pl.na_long, pl.ncb, pl.hb_slot,
             pl.anchor_pixels, (long long)pl.block_samples);
    o += b;
    o += " lv";
    for (int i = 0; i < s.n; ++i) snprintf(b, sizeof b, " %d:%d", pl.prow0[i], pl.abase[i]), o += b;
    o += " blk";
    for (int j = 0; j < pl.nblk; ++j) {
        const GatherPlanGroup &G = pl.blk[j];
        snprintf(b, sizeof b, " %d:%d,%d,%d,%d,%d", G.level, G.B, G.H, G.W, G.abase, G.first), o += b;
    }
    o += " anc";
    for (int j = 0; j < pl.nanc; ++j) {
        const GatherPlanGroup &G = pl.anc[j];
        snprintf(b, sizeof b, " %d:%d,%d,%d,%d,%d", G.level, G.B, G.H, G.W, G.abase, G.first), o += b;
    }
    return o;
}

// the fp32 kernels' part of both routes: the forward tile, the backward reduction slab, the LDS bytes of a refusal (0: served)
static std::string fp32_text(const DcnRoute &f, const DcnRoute &r)
{
    char b[128];
    snprintf(b, sizeof b, " | fp32 bn=%d red=%d over=%zu/%zu", f.fp32_bn, r.fp32_red, f.lds_over, r.lds_over);
    return b;
}

static int g_bad = 0;
// fp32: the row also states fp32_text (the rows of the KD thresholds; the others predate those fields and keep their texts)
static void expect(const char *name, const DcnRouteShape &s, const char *want, bool fp32 = false)
{
    const DcnRoute f = route_forward(s), r = route_backward(s);
    const std::string got = text(s, f, r) + (fp32 ? fp32_text(f, r) : std::string());
    printf("%s: %s/%s %s/%s %s", name, FWD[f.fwd], IMG[f.image], DATA[r.data], IMG[r.image], WG[r.wgrad]);
    if (got == want) {
        printf(" ok\n");
    } else {
        printf(" MISMATCH\n  got      %s\n  expected %s\n", got.c_str(), want);
        ++g_bad;
    }
}

int main()
{
    DcnRouteShape s;
    // ---- forward: mm -> grouped -> xn (planes with a workspace and 8 | C) -> fp32; pitched / prepared only channels-last on FWD_MM ----
    s = shape(64, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    expect("fwd 3x3 64->128", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    s.gather_ws = false, s.gather_ws_bytes = 0, s.nchw = true;
    expect("fwd 3x3 64->128 reference layout", s,
           "fwd=0 image=1 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=0 pitched=0 gcol_ks=0 own=1 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 192, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 884736, 737280);
    expect("fwd 3x3 64->192", s,
           "fwd=2 image=2 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(48, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 393216);
    expect("fwd 3x3 48->128", s,
           "fwd=2 image=2 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,763904,764416,766464,782592,846336,973824,1360896,1424640 bytes=1488384 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    s.workspace = false;
    expect("fwd 3x3 64->128 no workspace", s,
           "fwd=3 image=0 pitched=0 prepared=0 vec=1 | data=5 image=0 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0");
    s = shape(68, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 663552, 491520);
    expect("fwd 3x3 68->128", s,
           "fwd=3 image=0 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1082112,1082624,1084672,1100800,1164544,1292032,1840384,1904128 bytes=1967872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 64, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 221184, 245760);
    expect("fwd 3x3 64->64", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(66, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 663552, 491520);
    expect("fwd 3x3 66->128", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=0 | data=5 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0");
    s = shape(64, 128, 3, 3, 1, 1, {L0});
    kernels(s, 0, 0, 18432, 18432, 25344, 26624, 0, 0);
    expect("fwd 3x3 64->128 exact mode", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=32 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    s.general_gemms = true;
    expect("fwd 3x3 64->128 general-gemms bit", s,
           "fwd=2 image=2 pitched=0 prepared=0 vec=1 | data=3 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1228288,1292032 bytes=1355776 NB=40 NA=0 na_long=0 ncb=1 hb_slot=15912 apx=0 bs=3978 lv 0:0 blk 0:2,13,17,0,0 anc");
    s = shape(512, 512, 3, 3, 64, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 14155776, 14155776);
    expect("fwd 3x3 512->512 64 groups", s,
           "fwd=1 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=4 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,8146944,8147456,8149504,8165632,8229376,8356864,12485632,12613120 bytes=12676864 NB=0 NA=504 na_long=0 ncb=2 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(1024, 1024, 3, 3, 64, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 56623104, 56623104);
    expect("fwd 3x3 1024->1024 64 groups", s,
           "fwd=1 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=4 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,16293888,16294400,16296448,16312576,16376320,16503808,24761344,25016064 bytes=25079808 NB=0 NA=504 na_long=0 ncb=4 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(2048, 2048, 3, 3, 64, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 226492416, 226492416);
    expect("fwd 3x3 2048->2048 64 groups", s,
           "fwd=1 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=8 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,32587776,32588288,32590336,32606464,32670208,32797696,49312768,49821952 bytes=49885696 NB=0 NA=504 na_long=0 ncb=8 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(256, 256, 3, 3, 64, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 3538944, 3538944);
    expect("fwd 3x3 256->256 64 groups (4 per group)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=4 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,4073472,4073984,4076032,4092160,4155904,4283392,6347776,6411520 bytes=6475264 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 128, 4, 7, 1, 1, {L0});
    kernels(s, 6, 3, 81920, 180224, 128000, 46080, 1376256, 1376256);
    expect("fwd 4x7 64->128 (mm LDS at the cap)", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=12376 na=504 o=0,3168256,3169280,3171328,3220992,3419136,3815424,4331520,4529664 bytes=4727808 NB=0 NA=504 na_long=0 ncb=1 hb_slot=49504 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 128, 5, 6, 1, 1, {L0});
    kernels(s, 6, 3, 86016, 184320, 133632, 48128, 1474560, 1474560);
    expect("fwd 5x6 64->128 (mm LDS over the cap)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=13260 na=504 o=0,3394560,3395584,3397632,3450880,3663104,4087552,4603648,4815872 bytes=5028096 NB=0 NA=504 na_long=0 ncb=1 hb_slot=53040 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 192, 4, 5, 1, 1, {L0});
    kernels(s, 6, 3, 65536, 163840, 105472, 37888, 1966080, 1474560);
    expect("fwd 4x5 64->192 (xn LDS at the cap)", s,
           "fwd=2 image=2 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=8840 na=504 o=0,2263040,2263808,2265856,2301440,2443008,2726144,3242240,3383808 bytes=3525376 NB=0 NA=504 na_long=0 ncb=1 hb_slot=35360 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 192, 3, 7, 1, 1, {L0});
    kernels(s, 6, 3, 67584, 165888, 108288, 38912, 2064384, 1622016);
    expect("fwd 3x7 64->192 (xn LDS over the cap)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=9282 na=504 o=0,2376192,2376960,2379008,2416384,2565120,2862336,3378432,3527168 bytes=3675904 NB=0 NA=504 na_long=0 ncb=1 hb_slot=37128 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(512, 512, 5, 9, 64, 1, {L0});
    kernels(s, 6, 3, 116736, 215040, 175872, 63488, 70778880, 70778880);
    expect("fwd 5x9 512->512 64 groups (grouped LDS under the cap)", s,
           "fwd=1 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=4 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=19890 na=504 o=0,40734720,40736256,40738304,40817920,41136384,41773056,45901824,46538496 bytes=46856960 NB=0 NA=504 na_long=0 ncb=2 hb_slot=79560 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(512, 512, 6, 8, 64, 1, {L0});
    kernels(s, 6, 3, 122880, 221184, 184320, 66560, 75497472, 75497472);
    expect("fwd 6x8 512->512 64 groups (grouped LDS over the cap)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=4 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=21216 na=504 o=0,43450368,43451904,43453952,43538944,43878400,44557568,48686336,49365248 bytes=49704704 NB=0 NA=504 na_long=504 ncb=2 hb_slot=84864 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(8192, 4736, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 2095054848, 2095054848);
    expect("fwd 3x3 8192->4736 (fragment image below 2 GB)", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,130351104,130351616,130353664,130369792,130433536,130561024,196621312,198658048 bytes=198721792 NB=0 NA=504 na_long=0 ncb=32 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(8192, 4864, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 2151677952, 2151677952);
    expect("fwd 3x3 8192->4864 (fragment image above 2 GB)", s,
           "fwd=2 image=2 pitched=0 prepared=0 vec=1 | data=5 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0");
    // ---- backward data: gather grouped / mm / xn behind a gather workspace that holds the plan, else the scatter kernels ----
    s = shape(64, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    expect("bwd 3x3 64->128", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    s.workspace = false;
    expect("bwd 3x3 64->128 no workspace", s,
           "fwd=3 image=0 pitched=0 prepared=0 vec=1 | data=5 image=0 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0");
    s = shape(64, 512, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 1769472, 1966080);
    s.workspace = false;
    expect("bwd 3x3 64->512 no workspace", s,
           "fwd=3 image=0 pitched=0 prepared=0 vec=1 | data=5 image=0 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0");
    s = shape(64, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    s.gather_ws = false, s.gather_ws_bytes = 0;
    expect("bwd 3x3 64->128 no gather workspace", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=4 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0");
    s = shape(64, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    s.gather_ws = false, s.gather_ws_bytes = 0, s.nchw = true;
    expect("bwd 3x3 64->128 no gather workspace, reference layout", s,
           "fwd=0 image=1 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=0 pitched=0 gcol_ks=0 own=1 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    s.gather_ws_bytes = 1871872;
    expect("bwd 3x3 64->128 gather workspace of plan.bytes", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    s.gather_ws_bytes = 1871871;
    expect("bwd 3x3 64->128 gather workspace one byte short", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=4 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    s.atomic_scatter = true;
    expect("bwd 3x3 64->128 atomic-scatter bit", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=4 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0");
    s = shape(64, 128, 3, 3, 1, 1, {L0, {2, 13, 17, 13, 17, -1, true, false}});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    expect("bwd 3x3 64->128 offset gradients without grad_input beside a level with it", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=3 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=7956 na=504 o=0,2036736,2037504,2039552,2071552,2199040,2453760,2453760,2581248 bytes=2708736 NB=40 NA=0 na_long=0 ncb=1 hb_slot=31824 apx=0 bs=3978 lv 0:0 442:0 blk 0:2,13,17,0,0 anc");
    s = shape(64, 128, 3, 3, 1, 1, {{2, 13, 17, 13, 17, -1, true, true}});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    expect("bwd 3x3 64->128 no level with grad_input", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=4 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0");
    s = shape(64, 128, 3, 3, 1, 1, {{2, 13, 21, 25, 42, 0, true, false}, {2, 12, 21, 13, 21, 0, true, false}});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    expect("bwd 3x3 64->128 one grad_input, two shapes", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=4 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0");
    s = shape(64, 64, 3, 3, 1, 1, {L0});
    kernels(s, 0, 0, 18432, 18432, 25344, 26624, 0, 0);
    expect("bwd 3x3 64->64 exact mode", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=16 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 128, 3, 3, 1, 1, {L0});
    kernels(s, 0, 0, 18432, 18432, 25344, 26624, 0, 0);
    expect("bwd 3x3 64->128 exact mode", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=32 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 256, 3, 3, 1, 1, {L0});
    kernels(s, 0, 0, 18432, 18432, 25344, 26624, 0, 0);
    expect("bwd 3x3 64->256 exact mode", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=64 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 192, 3, 3, 1, 1, {L0});
    kernels(s, 0, 0, 18432, 18432, 25344, 26624, 0, 0);
    expect("bwd 3x3 64->192 exact mode", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 128, 3, 3, 1, 1, {L0});
    kernels(s, 0, 0, 18432, 18432, 25344, 26624, 0, 0);
    misalign_gout(s);
    expect("bwd 3x3 64->128 exact mode, grad_output at offset 8", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 66, 3, 3, 1, 1, {L0});
    kernels(s, 0, 0, 18432, 18432, 25344, 26624, 0, 0);
    expect("bwd 3x3 64->66 exact mode (pitch 66)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=0 | data=1 image=0 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(512, 512, 3, 3, 64, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 14155776, 14155776);
    expect("bwd 3x3 512->512 64 groups", s,
           "fwd=1 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=4 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,8146944,8147456,8149504,8165632,8229376,8356864,12485632,12613120 bytes=12676864 NB=0 NA=504 na_long=0 ncb=2 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(2048, 2048, 3, 3, 64, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 226492416, 226492416);
    expect("bwd 3x3 2048->2048 64 groups", s,
           "fwd=1 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=8 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,32587776,32588288,32590336,32606464,32670208,32797696,49312768,49821952 bytes=49885696 NB=0 NA=504 na_long=0 ncb=8 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 256, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 884736, 983040);
    s.gather_ws = false, s.gather_ws_bytes = 0;
    expect("bwd 3x3 64->256 no gather workspace", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=4 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0");
    s = shape(64, 264, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 1327104, 1105920);
    s.gather_ws = false, s.gather_ws_bytes = 0;
    expect("bwd 3x3 64->264 no gather workspace", s,
           "fwd=2 image=2 pitched=0 prepared=0 vec=1 | data=5 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0");
    s = shape(64, 252, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 884736, 983040);
    s.gather_ws = false, s.gather_ws_bytes = 0;
    expect("bwd 3x3 64->252 no gather workspace", s,
           "fwd=2 image=2 pitched=0 prepared=0 vec=1 | data=5 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0");
    s = shape(64, 128, 2, 5, 1, 1, {L0});
    kernels(s, 6, 3, 45056, 143360, 77312, 27648, 491520, 491520);
    s.gather_ws = false, s.gather_ws_bytes = 0;
    expect("bwd 2x5 64->128 no gather workspace (xn LDS under the cap)", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=4 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0");
    s = shape(64, 128, 3, 4, 1, 1, {L0});
    kernels(s, 6, 3, 49152, 147456, 82944, 29696, 589824, 589824);
    s.gather_ws = false, s.gather_ws_bytes = 0;
    expect("bwd 3x4 64->128 no gather workspace (xn LDS over the cap)", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=5 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0");
    // ---- the plan's two thresholds, strict inequalities, at equality and one step above; the channel blocks of the per-anchor sums ----
    s = shape(64, 128, 3, 3, 1, 1, {{1, 12, 12, 20, 20, 0, true, true}});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    s.general_gemms = true;
    expect("plan xn 12x12 <- 20x20 (3600 = 400 x 9 blocks)", s,
           "fwd=2 image=2 pitched=0 prepared=0 vec=1 | data=3 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3600 na=169 o=0,921600,921856,922624,937216,994816,1110272,1110272,1167872 bytes=1225472 NB=9 NA=0 na_long=0 ncb=1 hb_slot=14400 apx=0 bs=3600 lv 0:0 blk 0:1,12,12,0,0 anc");
    s = shape(64, 128, 3, 3, 1, 1, {{1, 12, 12, 20, 21, 0, true, true}});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    s.general_gemms = true;
    expect("plan xn 12x12 <- 20x21 (3780)", s,
           "fwd=2 image=2 pitched=0 prepared=0 vec=1 | data=3 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3780 na=169 o=0,967680,967936,968704,984064,1044736,1165824,1338880,1399552 bytes=1460224 NB=0 NA=169 na_long=169 ncb=1 hb_slot=15120 apx=144 bs=0 lv 0:0 blk anc 0:1,12,12,0,0");
    s = shape(64, 128, 3, 3, 1, 1, {{1, 8, 8, 18, 20, 0, true, true}});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    expect("plan mm 8x8 <- 18x20 (3240 = 40 x 81 anchors)", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3240 na=81 o=0,829440,829696,830208,843264,895232,999168,1082112,1134080 bytes=1186048 NB=0 NA=81 na_long=0 ncb=1 hb_slot=12960 apx=64 bs=0 lv 0:0 blk anc 0:1,8,8,0,0");
    s = shape(64, 128, 3, 3, 1, 1, {{1, 8, 8, 19, 20, 0, true, true}});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    expect("plan mm 8x8 <- 19x20 (3420)", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3420 na=81 o=0,875520,875776,876288,890112,944896,1054464,1137408,1192192 bytes=1246976 NB=0 NA=81 na_long=81 ncb=1 hb_slot=13680 apx=64 bs=0 lv 0:0 blk anc 0:1,8,8,0,0");
    s = shape(512, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 3538944, 3538944);
    expect("plan mm 512->128", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,8146944,8147456,8149504,8165632,8229376,8356864,12485632,12613120 bytes=12676864 NB=0 NA=504 na_long=0 ncb=2 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(512, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 3538944, 3538944);
    s.anchor_one_wave = true;
    expect("plan mm 512->128 one-wave bit", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,8146944,8147456,8149504,8165632,8229376,8356864,12485632,12613120 bytes=12676864 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(256, 256, 3, 3, 1, 1, {{2, 13, 21, 50, 84, 0, true, false}, {2, 25, 42, 25, 42, 1, true, false}, {2, 13, 21, 13, 21, 0, true, false}, {2, 13, 21, 7, 11, 0, true, false}});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 3538944, 3538944);
    expect("plan mm pyramid: three levels into one map, one into another", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=100800 na=2852 o=0,103219200,103232256,103243776,103646976,105259776,108485632,120167424,121780224 bytes=123393024 NB=0 NA=2852 na_long=616 ncb=1 hb_slot=403200 apx=2646 bs=0 lv 0:0 8400:616 10500:0 11046:0 blk anc 0:2,13,21,0,0 1:2,25,42,616,616");
    s = shape(256, 256, 3, 3, 1, 1, {{2, 13, 21, 50, 84, 0, true, false}, {2, 25, 42, 25, 42, 1, true, false}, {2, 13, 21, 13, 21, 0, true, false}});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 3538944, 3538944);
    s.general_gemms = true;
    expect("plan xn pyramid: a long and a short map", s,
           "fwd=2 image=2 pitched=0 prepared=0 vec=1 | data=3 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=99414 na=2852 o=0,101799936,101812736,101824256,102222080,103812864,106994176,109517312,111108096 bytes=112698880 NB=154 NA=616 na_long=616 ncb=1 hb_slot=397656 apx=546 bs=18900 lv 0:0 8400:616 10500:0 blk 1:2,25,42,616,0 anc 0:2,13,21,0,0");
    // ---- weight gradient: grouped -> mm (needs the gather pass's tap table, 16-byte aligned) -> the split kernels with their grid ----
    s = shape(512, 512, 3, 3, 64, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 14155776, 14155776);
    s.want_wgrad = true;
    expect("wgrad 3x3 512->512 64 groups", s,
           "fwd=1 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=4 own=0 wgrad=1 wg_steps=14 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,8146944,8147456,8149504,8165632,8229376,8356864,12485632,12613120 bytes=12676864 NB=0 NA=504 na_long=0 ncb=2 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(256, 256, 3, 3, 64, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 3538944, 3538944);
    s.want_wgrad = true;
    expect("wgrad 3x3 256->256 64 groups (4 per group)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=4 own=0 wgrad=1 wg_steps=14 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,4073472,4073984,4076032,4092160,4155904,4283392,6347776,6411520 bytes=6475264 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(512, 512, 5, 5, 64, 1, {L0});
    kernels(s, 6, 3, 75776, 174080, 119552, 43008, 39321600, 39321600);
    s.want_wgrad = true;
    expect("wgrad 5x5 512->512 64 groups", s,
           "fwd=1 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=4 own=0 wgrad=3 wg_steps=14 grid=1600/1/1 | plan ok=1 ns=11050 na=504 o=0,22630400,22631424,22633472,22677760,22854656,23208448,27337216,27691008 bytes=27867904 NB=0 NA=504 na_long=0 ncb=2 hb_slot=44200 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 256, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 884736, 983040);
    s.want_wgrad = true;
    expect("wgrad 3x3 64->256", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=2 wg_steps=14 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 256, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 884736, 983040);
    s.gather_ws_aligned16 = false, s.want_wgrad = true;
    expect("wgrad 3x3 64->256 gather workspace at offset 4", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=2 image=1 prepared=1 pitched=0 gcol_ks=0 own=0 wgrad=3 wg_steps=14 grid=9/1/14 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 256, 3, 3, 1, 1, {{2, 13, 17, 13, 17, -1, false, false}});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 884736, 983040);
    s.want_wgrad = true;
    expect("wgrad 3x3 64->256 no data gradient", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=0 image=0 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=3 wg_steps=14 grid=9/1/14 | plan ok=0");
    s = shape(64, 128, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    s.want_wgrad = true;
    expect("wgrad 3x3 64->128", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=2 image=1 prepared=1 pitched=0 gcol_ks=0 own=0 wgrad=3 wg_steps=14 grid=9/1/14 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(6, 27, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 55296, 12288);
    s.want_wgrad = true;
    expect("wgrad 3x3 6->27", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=0 | data=5 image=0 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=4 wg_steps=14 grid=9/1/14 | plan ok=0");
    s = shape(6, 27, 3, 3, 1, 1, {L0});
    kernels(s, 0, 0, 18432, 18432, 25344, 26624, 0, 0);
    s.want_wgrad = true;
    expect("wgrad 3x3 6->27 exact mode", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=0 | data=5 image=0 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=6 wg_steps=14 grid=9/1/14 | plan ok=0");
    s = shape(2048, 3640, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 410517504, 403439616);
    s.want_wgrad = true;
    expect("wgrad 3x3 2048->3640 (ordered reduce at 256 MB)", s,
           "fwd=2 image=2 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=1 pitched=0 gcol_ks=0 own=0 wgrad=3 wg_steps=14 grid=288/15/1 | plan ok=1 ns=3978 na=504 o=0,32587776,32588288,32590336,32606464,32670208,32797696,49312768,49821952 bytes=49885696 NB=0 NA=504 na_long=0 ncb=8 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(2048, 3644, 3, 3, 1, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 410517504, 403439616);
    s.want_wgrad = true;
    expect("wgrad 3x3 2048->3644 (ordered reduce above 256 MB)", s,
           "fwd=2 image=2 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=1 pitched=0 gcol_ks=0 own=0 wgrad=4 wg_steps=14 grid=288/15/1 | plan ok=1 ns=3978 na=504 o=0,32587776,32588288,32590336,32606464,32670208,32797696,49312768,49821952 bytes=49885696 NB=0 NA=504 na_long=0 ncb=8 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(64, 128, 3, 3, 1, 1, {L0});
    kernels(s, 0, 0, 18432, 18432, 25344, 26624, 0, 0);
    s.want_wgrad = true;
    expect("wgrad 3x3 64->128 exact mode", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=32 own=0 wgrad=5 wg_steps=14 grid=9/1/14 | plan ok=1 ns=3978 na=504 o=0,1018368,1018880,1020928,1037056,1100800,1228288,1744384,1808128 bytes=1871872 NB=0 NA=504 na_long=0 ncb=1 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0");
    s = shape(256, 256, 3, 3, 1, 1, {{2, 100, 168, 100, 168, 0, true, true}});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 3538944, 3538944);
    s.general_gemms = true, s.want_wgrad = true;
    expect("wgrad 3x3 256->256 tower 2x100x168, general-gemms bit", s,
           "fwd=2 image=2 pitched=0 prepared=0 vec=1 | data=3 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=3 wg_steps=1050 grid=36/1/14 | plan ok=1 ns=302400 na=34138 o=0,309657600,309810176,309946880,311156480,315994880,325671936,325671936,330510336 bytes=335348736 NB=2100 NA=0 na_long=0 ncb=1 hb_slot=1209600 apx=0 bs=302400 lv 0:0 blk 0:2,100,168,0,0 anc");
    s = shape(256, 256, 3, 3, 1, 1, {{2, 100, 168, 100, 168, 0, true, true}});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 3538944, 3538944);
    s.want_wgrad = true;
    expect("wgrad 3x3 256->256 tower 2x100x168", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=2 wg_steps=1050 grid=0/0/0 | plan ok=1 ns=302400 na=34138 o=0,309657600,309810176,309946880,311156480,315994880,325671936,465501184,470339584 bytes=475177984 NB=0 NA=34138 na_long=0 ncb=1 hb_slot=1209600 apx=33600 bs=0 lv 0:0 blk anc 0:2,100,168,0,0");
    // ---- the LDS thresholds cut in KD = kh kw dg, the largest count a kernel keeps and the next one (six products: npl = 3) ----
    // fwd_mm_lds = 8192 npl + 2048 KD <= 80 KiB: KD <= 28
    s = shape(64, 128, 2, 7, 1, 2, {L0});
    kernels(s, 6, 3, 81920, 180224, 128000, 31744, 688128, 688128);
    expect("kd 28 = 2x7 dg 2, 64->128 (fwd_mm_lds 81920 = the cap)", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=12376 na=504 o=0,1584128,1585152,1587200,1636864,1835008,2231296,2747392,2945536 bytes=3143680 NB=0 NA=504 na_long=0 ncb=1 hb_slot=49504 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0 | fp32 bn=0 red=0 over=0/0", true);
    s = shape(64, 128, 1, 29, 1, 1, {L0});
    kernels(s, 6, 3, 83968, 182272, 130816, 47104, 1425408, 1474560);
    expect("kd 29 = 1x29, 64->128 (fwd_mm_lds 83968)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=12818 na=504 o=0,3281408,3282432,3284480,3335936,3541248,3951616,4467712,4673024 bytes=4878336 NB=0 NA=504 na_long=0 ncb=1 hb_slot=51272 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0 | fp32 bn=256 red=0 over=0/0", true);
    // xn_lds = 40960 npl + 2048 KD <= 160 KiB: KD <= 20
    s = shape(64, 192, 2, 5, 1, 2, {L0});
    kernels(s, 6, 3, 65536, 163840, 105472, 27648, 983040, 737280);
    expect("kd 20 = 2x5 dg 2, 64->192 (xn_lds 163840 = the cap)", s,
           "fwd=2 image=2 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=8840 na=504 o=0,1131520,1132288,1134336,1169920,1311488,1594624,2110720,2252288 bytes=2393856 NB=0 NA=504 na_long=0 ncb=1 hb_slot=35360 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0 | fp32 bn=0 red=0 over=0/0", true);
    s = shape(64, 192, 1, 21, 1, 1, {L0});
    kernels(s, 6, 3, 67584, 165888, 108288, 38912, 2064384, 1622016);
    expect("kd 21 = 1x21, 64->192 (xn_lds 165888)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=9282 na=504 o=0,2376192,2376960,2379008,2416384,2565120,2862336,3378432,3527168 bytes=3675904 NB=0 NA=504 na_long=0 ncb=1 hb_slot=37128 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0 | fp32 bn=256 red=0 over=0/0", true);
    // bwd_xn_lds = 16384 npl + 2816 KD <= 80 KiB: KD <= 11
    s = shape(64, 128, 1, 11, 1, 1, {L0});
    kernels(s, 6, 3, 47104, 145408, 80128, 28672, 540672, 589824);
    s.gather_ws = false, s.gather_ws_bytes = 0;
    expect("kd 11 = 1x11, 64->128 no gather workspace (bwd_xn_lds 80128)", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=4 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0 | fp32 bn=0 red=0 over=0/0", true);
    s = shape(64, 128, 2, 3, 1, 2, {L0});
    kernels(s, 6, 3, 49152, 147456, 82944, 23552, 294912, 294912);
    s.gather_ws = false, s.gather_ws_bytes = 0;
    expect("kd 12 = 2x3 dg 2, 64->128 no gather workspace (bwd_xn_lds 82944)", s,
           "fwd=0 image=1 pitched=1 prepared=1 vec=1 | data=5 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0 | fp32 bn=0 red=256 over=0/0", true);
    // grouped weight gradient: kh kw <= 9
    s = shape(512, 512, 1, 9, 64, 1, {L0});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 14155776, 14155776);
    s.want_wgrad = true;
    expect("wgrad 1x9 512->512 64 groups (9 taps)", s,
           "fwd=1 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=4 own=0 wgrad=1 wg_steps=14 grid=0/0/0 | plan ok=1 ns=3978 na=504 o=0,8146944,8147456,8149504,8165632,8229376,8356864,12485632,12613120 bytes=12676864 NB=0 NA=504 na_long=0 ncb=2 hb_slot=15912 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0 | fp32 bn=0 red=0 over=0/0", true);
    s = shape(512, 512, 2, 5, 64, 1, {L0});
    kernels(s, 6, 3, 45056, 143360, 77312, 27648, 15728640, 15728640);
    s.want_wgrad = true;
    expect("wgrad 2x5 512->512 64 groups (10 taps)", s,
           "fwd=1 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=4 own=0 wgrad=3 wg_steps=14 grid=640/1/1 | plan ok=1 ns=4420 na=504 o=0,9052160,9052672,9054720,9072640,9143552,9285120,13413888,13555456 bytes=13626368 NB=0 NA=504 na_long=0 ncb=2 hb_slot=17680 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0 | fp32 bn=0 red=0 over=0/0", true);
    // ---- the fp32 kernels, last of their pass: the 256-wide tile while the tap table leaves room for it, then the 64-wide one,
    // then -- backward only, kh kw dg <= 64 -- the refusal.  fwd_fp32_lds = 33 x 4 (64 + BN) + 2048 KD, bwd_fp32_lds = 128 RED + 2816 KD ----
    s = shape(64, 192, 1, 59, 1, 1, {L0});
    kernels(s, 6, 3, 145408, 243712, 215296, 77824, 5799936, 4423680);
    expect("kd 59 = 1x59, 64->192 (fwd_fp32_lds 256-wide 163072)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=26078 na=504 o=0,6675968,6677760,6679808,6784256,7201536,8036096,8552192,8969472 bytes=9386752 NB=0 NA=504 na_long=504 ncb=1 hb_slot=104312 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0 | fp32 bn=256 red=0 over=0/0", true);
    s = shape(64, 192, 6, 10, 1, 1, {L0});
    kernels(s, 6, 3, 147456, 245760, 218112, 78848, 5898240, 4423680);
    expect("kd 60 = 6x10, 64->192 (fwd_fp32_lds 256-wide 165120, 64-wide 139776)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=26520 na=504 o=0,6789120,6790912,6792960,6899200,7323648,8172544,8688640,9113088 bytes=9537536 NB=0 NA=504 na_long=504 ncb=1 hb_slot=106080 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0 | fp32 bn=64 red=0 over=0/0", true);
    s = shape(64, 128, 2, 23, 1, 1, {L0});
    kernels(s, 6, 3, 118784, 217088, 178688, 64512, 2260992, 2260992);
    s.gather_ws = false, s.gather_ws_bytes = 0;
    expect("kd 46 = 2x23, 64->128 no gather workspace (bwd_fp32_lds 256-wide 162304)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=5 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0 | fp32 bn=256 red=256 over=0/0", true);
    s = shape(64, 128, 1, 47, 1, 1, {L0});
    kernels(s, 6, 3, 120832, 219136, 181504, 65536, 2310144, 2359296);
    s.gather_ws = false, s.gather_ws_bytes = 0;
    expect("kd 47 = 1x47, 64->128 no gather workspace (bwd_fp32_lds 256-wide 165120, 64-wide 140544)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=5 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0 | fp32 bn=256 red=64 over=0/0", true);
    s = shape(64, 128, 5, 11, 1, 1, {L0});
    kernels(s, 6, 3, 137216, 235520, 204032, 73728, 2703360, 2752512);
    s.gather_ws = false, s.gather_ws_bytes = 0;
    expect("kd 55 = 5x11, 64->128 no gather workspace (bwd_fp32_lds 64-wide 163072: the last count every route serves)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=5 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0 | fp32 bn=256 red=64 over=0/0", true);
    s = shape(64, 128, 7, 8, 1, 1, {L0});
    kernels(s, 6, 3, 139264, 237568, 206848, 74752, 2752512, 2752512);
    s.gather_ws = false, s.gather_ws_bytes = 0;
    expect("kd 56 = 7x8, 64->128 no gather workspace (bwd_fp32_lds 64-wide 165888: refused)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=5 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0 | fp32 bn=256 red=64 over=0/165888", true);
    s = shape(64, 128, 7, 8, 1, 1, {L0});
    kernels(s, 6, 3, 139264, 237568, 206848, 74752, 2752512, 2752512);
    expect("kd 56 = 7x8, 64->128 (the gather route serves it)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=2 image=1 prepared=1 pitched=1 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=24752 na=504 o=0,6336512,6338304,6340352,6439424,6835456,7627776,8143872,8539904 bytes=8935936 NB=0 NA=504 na_long=504 ncb=1 hb_slot=99008 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0 | fp32 bn=256 red=0 over=0/0", true);
    s = shape(32, 32, 8, 8, 1, 1, {L0});
    kernels(s, 6, 3, 155648, 253952, 229376, 82944, 393216, 393216);
    s.atomic_scatter = true;
    expect("kd 64 = 8x8, 32->32 atomic-scatter bit (fwd_fp32_lds 64-wide 147968; bwd_fp32_lds 188416: refused)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=5 image=3 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=0 | fp32 bn=64 red=64 over=0/188416", true);
    s = shape(32, 32, 8, 8, 1, 1, {L0});
    kernels(s, 0, 0, 131072, 131072, 180224, 82944, 0, 0);
    expect("kd 64 = 8x8, 32->32 exact mode (the grouped gather serves it)", s,
           "fwd=4 image=0 pitched=0 prepared=0 vec=1 | data=1 image=0 prepared=0 pitched=0 gcol_ks=0 own=0 wgrad=0 wg_steps=0 grid=0/0/0 | plan ok=1 ns=28288 na=504 o=0,3620864,3622912,3624960,3738112,4190720,5096192,5354240,5806848 bytes=6259456 NB=0 NA=504 na_long=504 ncb=1 hb_slot=113152 apx=442 bs=0 lv 0:0 blk anc 0:2,13,17,0,0 | fp32 bn=64 red=0 over=0/0", true);
    // ---- gather_plan directly: 2^27 pixel rows of nine samples are 9 x 2^27 >= 2^30 samples (no route reaches the plan with them) ----
    s = shape(64, 128, 3, 3, 1, 1, {{1, 8, 8, 8192, 16384, 0, true, true}});
    kernels(s, 6, 3, 43008, 141312, 74496, 26624, 442368, 491520);
    const bool refused = !gather_plan(s, true).ok && !gather_plan(s, false).ok;
    printf("plan direct 8x8 <- 8192x16384 (9 x 2^27 samples): %s\n", refused ? "refused ok" : "planned MISMATCH, expected a refusal");
    g_bad += refused ? 0 : 1;
    return g_bad ? 1 : 0;
}
