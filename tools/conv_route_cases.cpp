// The route of a dense convolution launch and the stream-K piece planner (lsnet_amd/csrc/conv_route.h) on the host, without a GPU:
// one line per case, "<name>: <result> ok" or "... MISMATCH, expected <result>", and a non-zero exit status when a case misses
// its row.  tests/test_conv_route_host.py builds this with g++ under the address and undefined-behaviour sanitizers.
// A result reads "<tile> <pixel tiles>x<column blocks> ks=<splits> dp=<whole tiles> sk=<pieces>/<their tiles>" or "refused".
// The expectations were taken from the rules as they stood in conv.hip and dcn.hip before this header existed (sk_plan, z_split,
// dcn_sk_plan, the tile codes of conv_forward), not from the header.  One branch of the planner has no row: "no more pieces than
// tiles" cannot happen, since a reduction of 8 chunks gets two pieces per tile and min(2 r, 512) > r for every r <= 448.
#include <stdio.h>
#include <string.h>

#include "conv_route.h"

static const char *TILES[] = {"128x32", "128x64", "64x128", "64x128_UNAL", "64x256", "64x256_ROWS"};
static const char *FWD_REFUSAL = "conv2d: C % 4 != 0 needs more than 64 output channels";
static const char *BWD_REFUSAL = "conv2d backward-data: Co % 4 != 0 needs C > 64";

// C input channels of the GEMM (the reduction), Co its output columns, P0 / P1 the output pixels of one or two levels
static ConvRouteShape shape(int C, int Co, int taps, int P0, int P1 = 0)
{
    ConvRouteShape s = {};
    s.n = P1 ? 2 : 1, s.P[0] = P0, s.P[1] = P1;
    s.C = s.xpitch = C, s.Co = Co, s.taps = taps;
    return s;
}
static ConvRouteShape pitch(ConvRouteShape s, int xpitch) { return s.xpitch = xpitch, s; }
static ConvRouteShape dgrad(ConvRouteShape s) { return s.data_grad = true, s; }                  // stride 1: a dense output
static ConvRouteShape cls(ConvRouteShape s) { return s.data_grad = s.ostep = true, s; }          // a residue class of a strided one
static ConvRouteShape rows(ConvRouteShape s, bool rows32) { return s.rows_gemm = true, s.rows32 = rows32, s; }

static int g_bad = 0;
static void report(const char *name, const char *got, const char *want)
{
    if (strcmp(got, want) == 0) {
        printf("%s: %s ok\n", name, got);
    } else {
        printf("%s: %s MISMATCH, expected %s\n", name, got, want);
        ++g_bad;
    }
}

static void route(const char *name, const ConvRouteShape &s, ConvTile tile, int tiles, int colblocks, int ks, int n_dp, int sk_n, int sk_tiles)
{
    static const int BM[] = {128, 128, 64, 64, 64, 64}, BN[] = {32, 64, 128, 128, 256, 256};
    const ConvRoute r = conv_route(s);
    char got[160], want[160];
    if (r.unsupported) snprintf(got, sizeof(got), "refused (%s)", r.unsupported);
    else
        snprintf(got, sizeof(got), "%s %dx%d ks=%d dp=%d sk=%d/%d%s", TILES[r.tile], r.tiles, r.colblocks, r.ks, r.sk.n_dp, r.sk.sk_n,
                 r.sk.sk_tiles, r.bm == BM[r.tile] && r.bn == BN[r.tile] ? "" : " (bm x bn is not the tile's)");
    snprintf(want, sizeof(want), "%s %dx%d ks=%d dp=%d sk=%d/%d", TILES[tile], tiles, colblocks, ks, n_dp, sk_n, sk_tiles);
    report(name, got, want);
}

static void refused(const char *name, const ConvRouteShape &s, const char *why)
{
    const ConvRoute r = conv_route(s);
    char got[160], want[160];
    if (r.unsupported) snprintf(got, sizeof(got), "refused (%s)", r.unsupported);
    else snprintf(got, sizeof(got), "%s", TILES[r.tile]);
    snprintf(want, sizeof(want), "refused (%s)", why);
    report(name, got, want);
}

static void pieces(const char *name, const SkPieces &p, int n_dp, int sk_n, int sk_tiles)
{
    char got[64], want[64];
    snprintf(got, sizeof(got), "dp=%d sk=%d/%d", p.n_dp, p.sk_n, p.sk_tiles);
    snprintf(want, sizeof(want), "dp=%d sk=%d/%d", n_dp, sk_n, sk_tiles);
    report(name, got, want);
}

static void split(const char *name, int ntw, int Tall, int ks)
{
    char got[32], want[32];
    snprintf(got, sizeof(got), "ks=%d", z_split(ntw, Tall));
    snprintf(want, sizeof(want), "ks=%d", ks);
    report(name, got, want);
}

int main()
{
    // ---- tiles
    route("1x1 64->32 8192 px", shape(64, 32, 1, 8192), CT_128x32, 64, 1, 1, 64, 0, 0);
    route("1x1 64->33 8192 px", shape(64, 33, 1, 8192), CT_128x64, 64, 1, 1, 64, 0, 0);
    route("1x1 64->64 8192 px", shape(64, 64, 1, 8192), CT_128x64, 64, 1, 1, 64, 0, 0);
    route("1x1 64->65 8192 px", shape(64, 65, 1, 8192), CT_64x128, 128, 1, 1, 128, 0, 0);
    route("1x1 64->256 32704 px (511 blocks of 64x256)", shape(64, 256, 1, 511 * 64), CT_64x128, 511, 2, 1, 1022, 0, 0);
    route("1x1 64->256 32705 px (512 blocks of 64x256)", shape(64, 256, 1, 511 * 64 + 1), CT_64x256, 512, 1, 1, 512, 0, 0);
    route("1x1 64->512 16320 px (510 blocks of 64x256)", shape(64, 512, 1, 255 * 64), CT_64x128, 255, 4, 1, 1020, 0, 0);
    route("1x1 64->512 16321 px (512 blocks of 64x256)", shape(64, 512, 1, 255 * 64 + 1), CT_64x256, 256, 2, 1, 512, 0, 0);
    route("3x3 64->256 8192 px", shape(64, 256, 9, 8192), CT_64x256, 128, 1, 1, 0, 512, 128);
    route("3x3 64->384 8192 px", shape(64, 384, 9, 8192), CT_64x128, 128, 3, 1, 0, 512, 384);
    // ---- alignment
    refused("3x3 27->64 8192 px", shape(27, 64, 9, 8192), FWD_REFUSAL);
    refused("3x3 27->32 8192 px", shape(27, 32, 9, 8192), FWD_REFUSAL);
    route("3x3 27->65 8192 px", shape(27, 65, 9, 8192), CT_64x128_UNAL, 128, 1, 1, 0, 256, 128);
    route("3x3 27->256 8192 px", shape(27, 256, 9, 8192), CT_64x128_UNAL, 128, 2, 1, 0, 512, 256);
    route("1x1 27->256 40000 px (625 blocks of 64x256)", shape(27, 256, 1, 40000), CT_64x128_UNAL, 625, 2, 1, 1250, 0, 0);
    refused("3x1 row-merged 12 (pitch 6)->64 8192 px", pitch(shape(12, 64, 3, 8192), 6), FWD_REFUSAL);
    route("3x1 row-merged 12 (pitch 6)->256 8192 px", pitch(shape(12, 256, 3, 8192), 6), CT_64x128_UNAL, 128, 2, 1, 256, 0, 0);
    route("7x1 row-merged 28 (pitch 4)->64 8192 px", pitch(shape(28, 64, 7, 8192), 4), CT_128x64, 64, 1, 1, 64, 0, 0);
    refused("data gradient of 3x3 64->27 8192 px", dgrad(shape(27, 64, 9, 8192)), BWD_REFUSAL);
    route("data gradient of 3x3 65->27 8192 px", dgrad(shape(27, 65, 9, 8192)), CT_64x128_UNAL, 128, 1, 1, 0, 256, 128);
    route("data gradient of 3x3 256->27 2x100x168", dgrad(shape(27, 256, 9, 2 * 100 * 168)), CT_64x128_UNAL, 525, 2, 1, 1050, 0, 0);
    route("data gradient of 3x3 s2 256->27, class of 4 taps, 2x13x21", cls(shape(27, 256, 4, 2 * 13 * 21)), CT_64x128_UNAL, 9, 2, 1, 18, 0, 0);
    refused("data gradient of 3x3 s2 52->27, class of 1 tap, 1x12x16", cls(shape(27, 52, 1, 12 * 16)), BWD_REFUSAL);
    // ---- blockIdx.z splits inside a route
    route("3x3 2048->256 1x13x21", shape(2048, 256, 9, 13 * 21), CT_64x256, 5, 1, 16, 5, 0, 0);
    route("3x3 256->256 2x13x21 + 2x7x11: two levels", shape(256, 256, 9, 2 * 13 * 21, 2 * 7 * 11), CT_64x256, 12, 1, 1, 0, 48, 12);
    route("3x3 256->256 2x13x21 alone", shape(256, 256, 9, 2 * 13 * 21), CT_64x256, 9, 1, 9, 9, 0, 0);
    route("data gradient of 3x3 s2 256->256, class of 4 taps, 2x13x21: an output step", cls(shape(256, 256, 4, 2 * 13 * 21)), CT_64x256, 9, 1, 1, 0, 36, 9);
    route("the same class as a dense output", dgrad(shape(256, 256, 4, 2 * 13 * 21)), CT_64x256, 9, 1, 4, 9, 0, 0);
    // ---- the rows GEMM of the deformable backward
    route("rows 256 -> 9 x 256 columns, 2100 + 546 rows", rows(shape(256, 2304, 1, 2100, 546), true), CT_64x256_ROWS, 42, 9, 1, 378, 0, 0);
    route("rows 256 -> 9 x 256 columns, 16800 rows", rows(shape(256, 2304, 1, 16800), true), CT_64x256_ROWS, 263, 9, 1, 2367, 0, 0);
    route("rows 256 -> 9 x 256 columns, 16800 rows beyond 32-bit offsets", rows(shape(256, 2304, 1, 16800), false), CT_64x256, 263, 9, 1, 2367, 0, 0);
    route("rows 256 -> 9 x 256 columns, 2100 rows beyond 32-bit offsets", rows(shape(256, 2304, 1, 2100), false), CT_64x128, 33, 18, 1, 512, 164, 82);
    route("rows 64 -> 9 x 64 columns, 16800 rows", rows(shape(64, 576, 1, 16800), true), CT_64x128, 263, 5, 1, 1315, 0, 0);
    route("rows 64 -> 9 x 64 columns, 546 rows", rows(shape(64, 576, 1, 546), true), CT_64x128, 9, 5, 1, 45, 0, 0);
    // ---- tests/test_stream_state_gpu.py
    route("Z_SPLIT forward: 3x3 256->64 1x8x8", shape(256, 64, 9, 64), CT_128x64, 1, 1, 9, 1, 0, 0);
    route("Z_SPLIT data gradient", dgrad(shape(64, 256, 9, 64)), CT_64x256, 1, 1, 2, 1, 0, 0);
    route("STREAM_K forward: 3x3 64->128 2x65x64", shape(64, 128, 9, 2 * 65 * 64), CT_64x128, 130, 1, 1, 0, 512, 130);
    route("STREAM_K data gradient", dgrad(shape(128, 64, 9, 2 * 65 * 64)), CT_128x64, 65, 1, 4, 65, 0, 0);
    // ---- tests/test_ops_gpu.py test_conv2d_stream_k_is_deterministic (B = 2)
    route("3x3 512->512 2x25x42 forward", shape(512, 512, 9, 2 * 25 * 42), CT_64x256, 33, 2, 7, 66, 0, 0);
    route("3x3 512->512 2x25x42 data gradient", dgrad(shape(512, 512, 9, 2 * 25 * 42)), CT_64x256, 33, 2, 7, 66, 0, 0);
    route("3x3 256->256 2x50x84 forward", shape(256, 256, 9, 2 * 50 * 84), CT_64x256, 132, 1, 1, 0, 512, 132);
    route("3x3 256->256 2x50x84 data gradient", dgrad(shape(256, 256, 9, 2 * 50 * 84)), CT_64x256, 132, 1, 1, 0, 512, 132);
    route("3x3 192->512 2x130x130 forward", shape(192, 512, 9, 2 * 130 * 130), CT_64x256, 529, 2, 1, 1058, 0, 0);
    route("3x3 192->512 2x130x130 data gradient", dgrad(shape(512, 192, 9, 2 * 130 * 130)), CT_64x128, 529, 2, 1, 1058, 0, 0);
    route("3x3 192->512 2x92x92 forward", shape(192, 512, 9, 2 * 92 * 92), CT_64x256, 265, 2, 1, 512, 234, 18);
    route("3x3 192->512 2x92x92 data gradient", dgrad(shape(512, 192, 9, 2 * 92 * 92)), CT_64x128, 265, 2, 1, 512, 288, 18);
    route("3x3 s2 256->256 2x100x168 forward", shape(256, 256, 9, 2 * 50 * 84), CT_64x256, 132, 1, 1, 0, 512, 132);
    route("3x3 s2 256->256 2x100x168 data gradient, class of 1 tap", cls(shape(256, 256, 1, 2 * 50 * 84)), CT_64x128, 132, 2, 1, 0, 512, 264);
    route("3x3 s2 256->256 2x100x168 data gradient, classes of 2 taps", cls(shape(256, 256, 2, 2 * 50 * 84)), CT_64x256, 132, 1, 1, 0, 512, 132);
    route("3x3 s2 256->256 2x100x168 data gradient, class of 4 taps", cls(shape(256, 256, 4, 2 * 50 * 84)), CT_64x256, 132, 1, 1, 0, 512, 132);
    // ---- tests/test_ops_gpu.py CONV_CASES, the last four rows (the third and fourth are the rows above)
    route("3x3 192->512 1x130x130 forward", shape(192, 512, 9, 130 * 130), CT_64x256, 265, 2, 1, 512, 234, 18);
    route("3x3 192->512 1x130x130 data gradient", dgrad(shape(512, 192, 9, 130 * 130)), CT_64x128, 265, 2, 1, 512, 288, 18);
    route("3x3 64->512 1x184x182 forward", shape(64, 512, 9, 184 * 182), CT_64x256, 524, 2, 1, 1048, 0, 0);
    route("3x3 64->512 1x184x182 data gradient", dgrad(shape(512, 64, 9, 184 * 182)), CT_128x64, 262, 1, 1, 0, 512, 262);
    // ---- tests/conv_geometry_cases.py TILE_CO at 3x9x11
    route("3x3 72->24 3x9x11 forward", shape(72, 24, 9, 3 * 9 * 11), CT_128x32, 3, 1, 3, 3, 0, 0);
    route("3x3 72->48 3x9x11 forward", shape(72, 48, 9, 3 * 9 * 11), CT_128x64, 3, 1, 3, 3, 0, 0);
    route("3x3 72->136 3x9x11 forward", shape(72, 136, 9, 3 * 9 * 11), CT_64x128, 5, 2, 3, 10, 0, 0);
    route("3x3 72->256 3x9x11 forward", shape(72, 256, 9, 3 * 9 * 11), CT_64x256, 5, 1, 3, 5, 0, 0);
    route("1x1 32->256 3x9x11 forward", shape(32, 256, 1, 3 * 9 * 11), CT_64x128, 5, 2, 1, 10, 0, 0);
    route("3x3 72->24 3x9x11 data gradient", dgrad(shape(24, 72, 9, 3 * 9 * 11)), CT_64x128, 5, 1, 1, 0, 10, 5);
    route("3x3 32->136 3x9x11 data gradient", dgrad(shape(136, 32, 9, 3 * 9 * 11)), CT_128x32, 3, 1, 5, 3, 0, 0);
    // ---- z_split
    split("127 tiles, 16 chunks", 127, 16, 2);
    split("128 tiles, 16 chunks", 128, 16, 1);
    split("127 tiles, 15 chunks", 127, 15, 1);
    split("127 tiles, 144 chunks", 127, 144, 4);
    split("64 tiles, 144 chunks", 64, 144, 8);
    split("33 tiles, 144 chunks", 33, 144, 15);
    split("1 tile, 144 chunks: the cap of 16", 1, 144, 16);
    split("1 tile, 127 chunks: chunks / 8", 1, 127, 15);
    split("1 tile, 128 chunks: chunks / 8", 1, 128, 16);
    split("2 tiles, 72 chunks: chunks / 8", 2, 72, 9);
    split("1 tile, 16 chunks", 1, 16, 2);
    // ---- stream-K pieces, the dense rule
    pieces("130 tiles, 7 chunks", sk_pieces(130, 7, sk_admit_dense(130)), 130, 0, 0);
    pieces("130 tiles, 8 chunks", sk_pieces(130, 8, sk_admit_dense(130)), 0, 260, 130);
    pieces("130 tiles, 18 chunks", sk_pieces(130, 18, sk_admit_dense(130)), 0, 512, 130);
    pieces("1023 tiles, 18 chunks", sk_pieces(1023, 18, sk_admit_dense(1023)), 1023, 0, 0);
    pieces("1024 tiles, 18 chunks", sk_pieces(1024, 18, sk_admit_dense(1024)), 1024, 0, 0);
    pieces("1025 tiles, 18 chunks", sk_pieces(1025, 18, sk_admit_dense(1025)), 1025, 0, 0);
    pieces("512 tiles, 144 chunks: r = 0", sk_pieces(512, 144, sk_admit_dense(512)), 512, 0, 0);
    pieces("513 tiles, 144 chunks: sixteen pieces behind a round", sk_pieces(513, 144, sk_admit_dense(513)), 512, 16, 1);
    pieces("1 tile, 144 chunks: four pieces in a launch of its own", sk_pieces(1, 144, sk_admit_dense(1)), 0, 4, 1);
    pieces("448 tiles, 18 chunks: r = 448", sk_pieces(448, 18, sk_admit_dense(448)), 0, 512, 448);
    pieces("449 tiles, 18 chunks: r = 449", sk_pieces(449, 18, sk_admit_dense(449)), 449, 0, 0);
    pieces("960 tiles, 18 chunks: r = 448", sk_pieces(960, 18, sk_admit_dense(960)), 512, 512, 448);
    pieces("961 tiles, 18 chunks: r = 449", sk_pieces(961, 18, sk_admit_dense(961)), 961, 0, 0);
    pieces("1472 tiles, 18 chunks: r = 448 behind two rounds", sk_pieces(1472, 18, sk_admit_dense(1472)), 1472, 0, 0);
    pieces("448 tiles, 8 chunks: the fewest pieces per tile, 512 > r", sk_pieces(448, 8, sk_admit_dense(448)), 0, 512, 448);
    pieces("530 tiles, 54 chunks", sk_pieces(530, 54, sk_admit_dense(530)), 512, 234, 18);
    pieces("448 tiles, 9362 chunks: (U + 1) * 512 below 2^31", sk_pieces(448, 9362, sk_admit_dense(448)), 0, 512, 448);
    pieces("448 tiles, 9363 chunks: (U + 1) * 512 past 2^31", sk_pieces(448, 9363, sk_admit_dense(448)), 448, 0, 0);
    // ---- stream-K pieces, the deformable forward's rule
    pieces("255 tiles, 72 chunks", sk_pieces(255, 72, sk_admit_dcn_fwd(255, false, false)), 0, 512, 255);
    pieces("256 tiles, 72 chunks", sk_pieces(256, 72, sk_admit_dcn_fwd(256, false, false)), 256, 0, 0);
    pieces("700 tiles, 72 chunks", sk_pieces(700, 72, sk_admit_dcn_fwd(700, false, false)), 700, 0, 0);
    pieces("1023 tiles, 72 chunks", sk_pieces(1023, 72, sk_admit_dcn_fwd(1023, false, false)), 1023, 0, 0);
    pieces("1025 tiles, 72 chunks", sk_pieces(1025, 72, sk_admit_dcn_fwd(1025, false, false)), 1024, 16, 1);
    pieces("1024 tiles, 72 chunks: r = 0", sk_pieces(1024, 72, sk_admit_dcn_fwd(1024, false, false)), 1024, 0, 0);
    pieces("1472 tiles, 72 chunks: r = 448 behind two rounds", sk_pieces(1472, 72, sk_admit_dcn_fwd(1472, false, false)), 1024, 512, 448);
    pieces("2100 tiles, 72 chunks", sk_pieces(2100, 72, sk_admit_dcn_fwd(2100, false, false)), 2048, 512, 52);
    pieces("700 tiles, 72 chunks, forced", sk_pieces(700, 72, sk_admit_dcn_fwd(700, true, false)), 512, 512, 188);
    pieces("2100 tiles, 72 chunks, never", sk_pieces(2100, 72, sk_admit_dcn_fwd(2100, false, true)), 2100, 0, 0);
    pieces("100 tiles, 72 chunks, never", sk_pieces(100, 72, sk_admit_dcn_fwd(100, false, true)), 100, 0, 0);
    pieces("700 tiles, 72 chunks, forced and never", sk_pieces(700, 72, sk_admit_dcn_fwd(700, true, true)), 700, 0, 0);
    pieces("100 tiles, 7 chunks, forced", sk_pieces(100, 7, sk_admit_dcn_fwd(100, true, false)), 100, 0, 0);
    return g_bad ? 1 : 0;
}
