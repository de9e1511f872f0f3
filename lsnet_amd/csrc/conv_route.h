// How a dense convolution launch is tiled and its work divided: one function of the call's shape, plain C++ without HIP or library
// state, so that tools/conv_route_cases.cpp (tests/test_conv_route_host.py) compiles it on the host.  conv.hip fills the shape once
// per launch (forward, each residue class of a data gradient, the deformable backward GEMM), decides here and hands the ConvRoute
// to its one launcher, which does not ask again.  The stream-K piece planner below also serves the deformable forward (dcn.hip).
#pragma once

// pixels x output channels of a workgroup (conv_kernels.h conv_mm_kernel<TM, TN, WM, WN, ..>: (WM TM 32) x (WN TN 32))
enum ConvTile {
    CT_128x32,        // Co <= 32
    CT_128x64,        // Co <= 64
    CT_64x128,        // Co > 64, the fine MFMA / staging interleave
    CT_64x128_UNAL,   // ... C or the pixel pitch not a multiple of 4: guarded 4-byte slab loads (UNAL)
    CT_64x256,        // 256 | Co under a deep reduction or a full round
    CT_64x256_ROWS    // the deformable backward GEMM: 64 x 256 with whole-line stores (TRANS), plain output
};

constexpr int CR_MAXLV = 16;             // maps of one launch (conv.hip checks it is CV_MAXLV)
constexpr int CR_CHUNK = 32;             // reduction channels of one chunk (conv.hip checks cr_ncc against cv_ncc)
constexpr int CR_SK_MAX_TILES = 4096;    // arrival counters of a stream (conv.hip checks it is SK_MAX_TILES)
constexpr int CR_SLOTS = 512;            // workgroups of these kernels the chip holds at once: two per CU

constexpr int cr_ncc(int C) { return (C + CR_CHUNK - 1) / CR_CHUNK; }

struct ConvRouteShape {
    int n;              // levels
    int P[CR_MAXLV];    // output pixels of each
    int C, xpitch, Co, taps;
    bool ostep;         // the output is one residue class of a strided data gradient
    bool data_grad;     // (only words the refusal: C and Co are the GEMM's, i.e. the forward's Co and C)
    bool rows_gemm;     // conv_mm_rows: the deformable backward GEMM
    bool rows32;        // ... and its row blocks lie within 32-bit byte offsets
};

// Work distribution of one launch of W tiles.  The chip holds 512 workgroups, so the launch runs in ceil(W / 512) rounds and the
// last one is rarely full: 525 tiles (every convolution at the 100 x 168 maps of two images) cost 226 us against 177 us for 512
// (tools/ubench/tile_sweep), 132 or 33 tiles (stages 3 / 4) leave most of the chip idle.  Rounds 3 / 4 answered with a reduction
// split over blockIdx.z plus a reduce launch, and a second launch for the tail; both quantise again (the split rule produced 528
// workgroups for six layer shapes of the step).  Round 5, "stream-K": workgroups [0, n_dp) take one whole tile each -- every tile
// of the whole rounds -- and the r = W % 512 tiles of the last round are divided EVENLY BY CHUNKS over sk_n = min(r * per_tile,
// 512) further workgroups, per_tile = min(chunks / 4, cap) pieces per tile: a piece has about four chunks or more, with no
// guaranteed minimum (chunks / 4 rounds down).  cap is 4 in a launch of at most one round (the tile's last arriver adds the
// pieces on its own) and 16 for the few tiles behind a whole round (the chip is idle otherwise).
// No pieces for short reductions (< 8 chunks: the layer is bound by its output stream, and a partial tile costs what the tile
// costs), when the last round is empty or nearly full (r > 448), when the pieces would be no more than the tiles, and beyond
// the stream's arrival counters or the kernels' 32-bit unit arithmetic ((U + 1) * sk_n < 2^31, U = r * chunks).
struct SkPieces {
    int n_dp, sk_n, sk_tiles;
};

inline SkPieces sk_pieces(int ntw, int Tall, bool admitted)
{
    const SkPieces none = {ntw, 0, 0};
    if (!admitted || Tall < 8) return none;
    const int r = ntw % CR_SLOTS;
    if (r == 0 || r > 448) return none;
    int per_tile = Tall / 4;
    const int cap = ntw > CR_SLOTS ? 16 : 4;
    if (per_tile > cap) per_tile = cap;
    const long long pieces = (long long)r * per_tile;
    const int ns = pieces < CR_SLOTS ? (int)pieces : CR_SLOTS;
    if (ns <= r) return none;
    if (r > CR_SK_MAX_TILES || ((long long)r * Tall + 1) * ns >= ((long long)1 << 31)) return none;
    return SkPieces{ntw - r, ns, r};
}

// Which launches get pieces.  Dense: not from two whole rounds up -- such launches lose more to the segment loop's longer
// prologue in EVERY workgroup than the last round can return (profiles/r5_sk_policy.txt, layer-1 rows).
inline bool sk_admit_dense(int ntw) { return ntw < 2 * CR_SLOTS; }

// Deformable forward: the opposite between half a round and two rounds.  Measured (tools/ubench/dcn_step, LSN_DBG_FWD_SK_NEVER =
// whole tiles only, profiles/r6_dcn_sk.txt): the pyramid launch (2 100 tiles: four rounds and 52 tiles) 780 -> 759 us; the tower
// launch (700 tiles: one round and 188 tiles) 278 -> 283 us -- its second round runs one workgroup per CU, which has the matrix
// pipe to itself and finishes in ~0.65 of a round, so the even split has little to return and the pieces' table rebuild and
// hand-over cost more.  Launches of less than HALF a round (a backbone layer of configs 3 / 4: 8 400 pixels = 132 tiles, 2 100 =
// 33) leave most of the chip idle as whole tiles and take up to four pieces per tile, as the dense kernel's do.
// always / never: LSN_DBG_FWD_SK_ALWAYS (pieces for launches of any size: tests) / LSN_DBG_FWD_SK_NEVER.
inline bool sk_admit_dcn_fwd(int ntw, bool always, bool never)
{
    return !never && (always || ntw < CR_SLOTS / 2 || ntw >= 2 * CR_SLOTS);
}

// Fewer than 128 tiles under 16 chunks or more (stage 4, FPN P5 .. P7: 33 pixel tiles under 64 .. 144 chunks): with more than
// four pieces per tile the tile's last arriver would add eight partial tiles on its own while the chip idles -- these keep round
// 3's blockIdx.z split with its chip-wide reduce launch (profiles/r3_conv_ksplit.txt; forcing other split counts lost on every
// row of the round-4 sweep), rounded DOWN to one round of workgroups (round 3 / 4 rounded to nearest: 528 on 512 slots for six
// layer shapes of the step), at least eight chunks per split and at most 16 splits.
inline int z_split(int ntw, int Tall)
{
    if (ntw >= 128 || Tall < 16) return 1;
    int ks = CR_SLOTS / ntw;
    if (ks > Tall / 8) ks = Tall / 8;
    if (ks > 16) ks = 16;
    return ks < 1 ? 1 : ks;
}

struct ConvRoute {
    const char *unsupported;   // non-NULL: why no kernel serves the shape (nothing else is set then)
    ConvTile tile;
    int bm, bn;
    int tile0[CR_MAXLV];       // first pixel tile of each level
    int tiles, colblocks;      // pixel tiles of all levels; column blocks of bn output channels
    int ks;                    // > 1: blockIdx.z splits of the chunk range + the reduce launch (one dense level, no pieces)
    SkPieces sk;               // whole tiles and stream-K pieces (conv_kernels.h ConvArgs)
};

// Tile choice (two workgroups share a CU, so the chip holds 512 of them at once).  Round-4 sweep over the step's layer shapes
// (tools/ubench/conv_step, profiles/r4_conv_tiles.txt):
//   * 64 x 256 (a pixel slab is fetched and split ONCE for 256 output channels: half the split work per MFMA of the 128-wide
//     tiles) wins wherever Co is a multiple of 256 and the reduction is deep (more than one tap) or the launch fills a round
//     (round 5, with stream-K filling the chip either way: 64 x 256 for EVERY Co % 256 == 0 lost 3 % over the step's shapes,
//     forward 3944 -> 4078 us, data gradient 2871 -> 2959 us, tools/ubench/conv_step A/B -- the rule stands);
//   * 64 x 128 otherwise for Co > 64 -- the one tile with an unaligned-slab variant, so C % 4 != 0 or a pitch % 4 != 0 needs
//     Co > 64 and never gets 64 x 256; 128 x 64 / 128 x 32 for the narrow outputs;
//   * 128 x 128 lost on every row (fewer, longer workgroups) and the one-workgroup-per-CU fat register tiles (256 x 128,
//     128 x 256) lost by 30 %: both are gone.
// The deformable backward GEMM (N = K C columns, plain stores) takes the rows form of 64 x 256 whenever 256 | N and its
// epilogue's buffer descriptors reach every row block, as whole tiles in one split; otherwise it is routed like a 1x1 forward.
inline ConvRoute conv_route(const ConvRouteShape &s)
{
    ConvRoute r = {};
    const bool unal = s.C % 4 != 0 || s.xpitch % 4 != 0;
    if (unal && s.Co <= 64) {
        r.unsupported = s.data_grad ? "conv2d backward-data: Co % 4 != 0 needs C > 64"
                                    : "conv2d: C % 4 != 0 needs more than 64 output channels";
        return r;
    }
    auto tile = [&](ConvTile t, int bm, int bn) {
        r.tile = t, r.bm = bm, r.bn = bn, r.tiles = 0;
        for (int i = 0; i < s.n; ++i) r.tile0[i] = r.tiles, r.tiles += (s.P[i] + bm - 1) / bm;
        r.colblocks = (s.Co + bn - 1) / bn;
        return r.tiles * r.colblocks;
    };
    r.ks = 1;
    if (s.rows_gemm && s.Co % 256 == 0 && s.rows32) {
        r.sk = SkPieces{tile(CT_64x256_ROWS, 64, 256), 0, 0};
        return r;
    }
    int ntw;
    if (s.Co % 256 == 0 && !unal && (s.taps > 1 || tile(CT_64x256, 64, 256) >= CR_SLOTS)) ntw = tile(CT_64x256, 64, 256);
    else if (s.Co <= 32) ntw = tile(CT_128x32, 128, 32);
    else if (s.Co <= 64) ntw = tile(CT_128x64, 128, 64);
    else ntw = tile(unal ? CT_64x128_UNAL : CT_64x128, 64, 128);
    const int Tall = s.taps * cr_ncc(s.C);
    if (s.n == 1 && !s.ostep) r.ks = z_split(ntw, Tall);
    r.sk = sk_pieces(ntw, Tall, r.ks == 1 && sk_admit_dense(ntw));
    return r;
}
