// Detection decode of liblsnet_hip.so: per-level top-k, vector decode, threshold, ordering and greedy NMS of a whole batch.
#include "common.h"
#include "decode_rows.h"
#include "prof.h"

namespace lsn {

// ---------------------------------------------------------------------------------------------
// LSHead.get_bboxes (lsnet_amd/models/dense_heads/ls_head.py; lsnet_head.py:1439-1668, bbox_nms.py:60-99,
// nms_wrapper.py:119-157) for B images in three launches, the arithmetic in decode_rows.h:
//   1. decode_select_kernel, one workgroup per (level, image) whose level has more points than nms_pre: the points' keys
//      (order-preserving words of max-over-classes sigmoid) go to the workspace, a 4 x 8-bit radix select over LDS histograms
//      finds the nms_pre-th largest key, and two workgroup scans write the selected rows in ASCENDING row order -- every row
//      above the threshold key and the lowest rows equal to it.  A level with no more points than nms_pre takes all its rows
//      and needs no list.  An image's selected rows, level after level, are its `slots`.
//   2. decode_candidates_kernel, one lane per slot: the classes above score_thr append one 64-bit word each,
//      (~score key << 32 | slot * C + class), under an integer atomic counter; the slot's box is decoded once, stored by slot,
//      and its coordinates meet in an integer atomic max (bit patterns of non-negative floats order like the floats).
//      The words are all different and carry the whole order, so the order of arrival does not reach the result.
//   3. decode_nms_kernel, one workgroup per image: bitonic sort of the words (4096-word tiles in LDS, wider strides through
//      the workspace), then greedy NMS in chunks of 1024 candidates against a kept list in LDS that holds at most
//      max_per_img boxes -- a chunk is first tested against the kept list in parallel, then its survivors are taken in order,
//      three barriers per KEPT box -- and the kept rows are written: box, score, label and the vectors, decoded here from the
//      maps for the kept rows only.
// Nothing is allocated, nothing read back.  counts[b] < 0: more than cand_cap candidates, the image's rows are undefined.
// LSCPVHead.get_bboxes (lscpv_head.py; lscpvnet_head.py:905-1090) is the same three launches with one step changed: a level
// with a verification source has the corners of each candidate point's box snapped to the source's corner heat-map
// (decode_box_verified of decode_rows.h: 8 heat-map and 4 offset reads per point, no pooled map) before the box goes to
// `slotbox` and into the coordinate maximum.  It writes no vectors (nv = 0).
// ---------------------------------------------------------------------------------------------
constexpr int DECODE_MAX_IMAGES = 64, DECODE_MAX_LEVELS = 8, DECODE_MAX_KEEP = 2048, DECODE_TILE = 4096, DECODE_MAX_SOURCES = 8;

struct DecodeLv {
    const float *cls, *box, *vec;
    int64_t cs[4], bs[4], vs[4];   // element strides (batch, channel, y, x)
    int H, W;
    float stride;
    int select;     // 1: more points than nms_pre, rows come from the select list
    int slot_off;   // first slot of the level inside an image
    int key_off;    // first key of the level inside an image's key area (select levels only)
    int K;          // slots of the level
};

struct DecodeSrc {
    const float *heat, *off;   // corner heat-map logits (B, 2, H, W), sub-cell offsets (B, 4, H, W)
    int64_t hs[4], os[4];      // element strides (batch, channel, y, x)
    int H, W;
    float stride;
};

struct DecodeArgs {
    DecodeLv lv[DECODE_MAX_LEVELS];
    DecodeSrc src[DECODE_MAX_SOURCES];
    int verify[DECODE_MAX_LEVELS];   // the level's verification source, -1: decoded as it is
    float img_hw[DECODE_MAX_IMAGES][2];
    float sf[DECODE_MAX_IMAGES][4];
    int B, L, C, nv, kind, S, keys_per_image, cap, cap2, max_keep, class_agnostic;
    float score_thr, iou_thr;
    int *cnt;                  // [B] candidates seen
    unsigned *maxc;            // [B] bit pattern of the largest candidate coordinate
    unsigned *keys;            // [B][keys_per_image]
    int *sel;                  // [B][S]
    float *slotbox;            // [B][S][4]
    unsigned long long *cand;  // [B][cap2]
    float *dets, *vecs;
    int64_t *labels;
    int *counts;
};
static_assert(sizeof(DecodeArgs) <= 4096, "DecodeArgs is passed to the kernels by value");

// exclusive prefix sum over the 1024 threads of the workgroup; total: the sum.  tmp: 16 ints of LDS.
__device__ __forceinline__ int decode_scan(int v, int *tmp, int &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) tmp[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int t = tmp[i];
        base += i < w ? t : 0;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return base + inc - v;
}

__device__ __forceinline__ int decode_level_of(const DecodeArgs &a, int s)
{
    int l = 0;
    while (l + 1 < a.L && s >= a.lv[l + 1].slot_off) ++l;
    return l;
}

__device__ __forceinline__ DecodeGeom decode_geom(const DecodeArgs &a, int b, int l)
{
    DecodeGeom g;
    g.stride = a.lv[l].stride, g.img_h = a.img_hw[b][0], g.img_w = a.img_hw[b][1];
    for (int i = 0; i < 4; ++i) g.sf[i] = a.sf[b][i];
    return g;
}

__device__ __forceinline__ DecodeMap decode_map(const float *p, const int64_t *st, int b)
{
    DecodeMap m;
    m.base = p + (int64_t)b * st[0], m.sc = st[1], m.sy = st[2], m.sx = st[3];
    return m;
}

__global__ __launch_bounds__(1024) void decode_select_kernel(const DecodeArgs a)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix, s_remaining;
    __shared__ int tmp[16];
    const int tid = threadIdx.x, l = blockIdx.x, b = blockIdx.y;
    if (l == 0 && tid == 0) a.cnt[b] = 0, a.maxc[b] = 0u;
    const DecodeLv &lv = a.lv[l];
    if (!lv.select) return;
    const int P = lv.H * lv.W, K = lv.K;
    unsigned *keys = a.keys + (size_t)b * a.keys_per_image + lv.key_off;
    const DecodeMap cm = decode_map(lv.cls, lv.cs, b);
    // (the key is the maximum of the fp32 SCORES, as the torch statement takes it.  One sigmoid of the largest logit would give
    // the same key only if expf is monotone to its last bit, which nobody has checked for the device library: every class's
    // sigmoid is evaluated -- 710 us at C = 80 on the largest level, the price of that caution)
    for (int i = tid; i < P; i += 1024) {
        const int y = i / lv.W, x = i - y * lv.W;
        float best = decode_sigmoid(decode_at(cm, 0, y, x));
        for (int c = 1; c < a.C; ++c) best = decode_max(best, decode_sigmoid(decode_at(cm, c, y, x)));
        keys[i] = decode_key(best);
    }
    // the K-th largest key, byte by byte from the top: `prefix` holds the decided bytes, `remaining` how many of the rows
    // that share them are still wanted
    unsigned prefix = 0, remaining = (unsigned)K;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned himask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < P; i += 1024) {
            const unsigned key = keys[i];
            if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned rem = remaining, d = 255;
            for (;; --d) {
                if (hist[d] >= rem || d == 0) break;
                rem -= hist[d];
            }
            s_prefix = prefix | (d << shift), s_remaining = rem;
        }
        __syncthreads();
        prefix = s_prefix, remaining = s_remaining;
    }
    // rows with a key above `prefix`, and the first `remaining` rows equal to it, in ascending row order
    const int chunk = (P + 1023) / 1024, r0 = min(P, tid * chunk), r1 = min(P, r0 + chunk);
    int eq = 0;
    for (int i = r0; i < r1; ++i) eq += keys[i] == prefix;
    int total;
    int eqrank = decode_scan(eq, tmp, total);
    int take = 0;
    {
        int e = eqrank;
        for (int i = r0; i < r1; ++i) {
            const unsigned key = keys[i];
            take += key > prefix || (key == prefix && e++ < (int)remaining);
        }
    }
    int pos = decode_scan(take, tmp, total);
    int *sel = a.sel + (size_t)b * a.S + lv.slot_off;
    for (int i = r0; i < r1; ++i) {
        const unsigned key = keys[i];
        if ((key > prefix || (key == prefix && eqrank++ < (int)remaining)) && pos < K) sel[pos++] = i;
    }
}

__global__ __launch_bounds__(256) void decode_candidates_kernel(const DecodeArgs a)
{
    const int s = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (s >= a.S) return;
    const int l = decode_level_of(a, s);
    const DecodeLv &lv = a.lv[l];
    const int row = lv.select ? a.sel[(size_t)b * a.S + s] : s - lv.slot_off;
    if ((unsigned)row >= (unsigned)(lv.H * lv.W)) return;      // (never: the select fills all K rows of a level)
    const int y = row / lv.W, x = row - y * lv.W;
    const DecodeMap cm = decode_map(lv.cls, lv.cs, b);
    bool any = false;
    for (int c = 0; c < a.C; ++c) {
        const float score = decode_sigmoid(decode_at(cm, c, y, x));
        if (!(score > a.score_thr)) continue;
        any = true;
        const int idx = atomicAdd(&a.cnt[b], 1);
        if (idx < a.cap) a.cand[(size_t)b * a.cap2 + idx] = decode_order_key(score, (uint32_t)s * (uint32_t)a.C + (uint32_t)c);
    }
    if (!any) return;
    // the point's box, once and behind the class loop: the lanes of a wave meet their first candidate at different classes, and
    // inside the loop the wave would walk the decode (and a verification's chain of dependent reads) once per such class
    float box[4];
    const int v = a.verify[l];
    if (v < 0) {
        decode_box(decode_map(lv.box, lv.bs, b), a.kind == DECODE_VECTORS, a.nv, y, x, decode_geom(a, b, l), box);
    } else {
        const DecodeSrc &sr = a.src[v];
        DecodeCorner c;
        c.heat = decode_map(sr.heat, sr.hs, b), c.off = decode_map(sr.off, sr.os, b);
        c.H = sr.H, c.W = sr.W, c.stride = sr.stride;
        decode_box_verified(decode_map(lv.box, lv.bs, b), y, x, decode_geom(a, b, l), &c, box);
    }
    float *out = a.slotbox + ((size_t)b * a.S + s) * 4;
    unsigned m = 0;
    for (int i = 0; i < 4; ++i) {
        out[i] = box[i];
        const unsigned bits = box[i] > 0.f ? __float_as_uint(box[i]) : 0u;
        m = bits > m ? bits : m;
    }
    atomicMax(&a.maxc[b], m);
}

// one compare-exchange step of the bitonic network on words i and i + j of `w`; gi: the global index of word i
__device__ __forceinline__ void decode_cmpx(unsigned long long *w, int i, int j, int gi, int k)
{
    const unsigned long long x = w[i], y = w[i + j];
    const bool up = (gi & k) == 0;
    if ((x > y) == up) w[i] = y, w[i + j] = x;
}

__global__ __launch_bounds__(1024) void decode_nms_kernel(const DecodeArgs a)
{
    __shared__ unsigned long long tile[DECODE_TILE];            // the sort's tile, then the kept boxes (DECODE_MAX_KEEP x 4)
    __shared__ unsigned long long kept_key[DECODE_MAX_KEEP];
    __shared__ unsigned long long wmask[16];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int n = a.cnt[b];
    if (n > a.cap || n == 0) {
        if (tid == 0) a.counts[b] = n == 0 ? 0 : -1;
        return;
    }
    unsigned long long *g = a.cand + (size_t)b * a.cap2;
    int N2 = 1;
    while (N2 < n) N2 <<= 1;
    for (int i = n + tid; i < N2; i += 1024) g[i] = ~0ull;
    __syncthreads();
    // ---- sort, ascending
    const int m = N2 < DECODE_TILE ? N2 : DECODE_TILE;
    for (int base = 0; base < N2; base += DECODE_TILE) {
        for (int i = tid; i < m; i += 1024) tile[i] = g[base + i];
        __syncthreads();
        for (int k = 2; k <= m; k <<= 1)
            for (int j = k >> 1; j >= 1; j >>= 1) {
                for (int t = tid; t < m / 2; t += 1024) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    decode_cmpx(tile, i, j, base + i, k);
                }
                __syncthreads();
            }
        for (int i = tid; i < m; i += 1024) g[base + i] = tile[i];
        __syncthreads();
    }
    for (int k = DECODE_TILE * 2; k <= N2; k <<= 1) {
        for (int j = k >> 1; j >= DECODE_TILE; j >>= 1) {
            for (int t = tid; t < N2 / 2; t += 1024) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                decode_cmpx(g, i, j, i, k);
            }
            __syncthreads();
        }
        for (int base = 0; base < N2; base += DECODE_TILE) {
            for (int i = tid; i < DECODE_TILE; i += 1024) tile[i] = g[base + i];
            __syncthreads();
            for (int j = DECODE_TILE >> 1; j >= 1; j >>= 1) {
                for (int t = tid; t < DECODE_TILE / 2; t += 1024) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    decode_cmpx(tile, i, j, base + i, k);
                }
                __syncthreads();
            }
            for (int i = tid; i < DECODE_TILE; i += 1024) g[base + i] = tile[i];
            __syncthreads();
        }
    }
    // ---- greedy NMS: the first max_keep survivors in sorted order
    float(*kept)[4] = reinterpret_cast<float(*)[4]>(tile);
    const float maxc = __uint_as_float(a.maxc[b]);
    const float *slotbox = a.slotbox + (size_t)b * a.S * 4;
    int nk = 0;
    for (int base = 0; base < n && nk < a.max_keep; base += 1024) {
        const int i = base + tid;
        bool alive = i < n;
        unsigned long long key = 0;
        float bx[4] = {0.f, 0.f, 0.f, 0.f};
        if (alive) {
            key = g[i];
            const uint32_t id = decode_order_id(key), s = id / (uint32_t)a.C;
            const float off = a.class_agnostic ? 0.f : decode_nms_offset((int)(id - s * (uint32_t)a.C), maxc);
            for (int q = 0; q < 4; ++q) bx[q] = slotbox[(size_t)s * 4 + q] + off;
            for (int q = 0; q < nk && alive; ++q) alive = !decode_iou_gt(kept[q], bx, a.iou_thr);
        }
        for (;;) {
            const unsigned long long bal = __ballot(alive);
            if ((tid & 63) == 0) wmask[tid >> 6] = bal;
            __syncthreads();
            int first = -1;
            for (int w = 0; w < 16 && first < 0; ++w)
                if (wmask[w]) first = w * 64 + __ffsll((long long)wmask[w]) - 1;
            __syncthreads();
            if (first < 0) break;               // the same value in every thread
            if (tid == first) {
                for (int q = 0; q < 4; ++q) kept[nk][q] = bx[q];
                kept_key[nk] = key;
                alive = false;
            }
            ++nk;
            if (nk == a.max_keep) break;
            __syncthreads();
            if (alive && decode_iou_gt(kept[nk - 1], bx, a.iou_thr)) alive = false;
        }
    }
    __syncthreads();
    // ---- emit
    if (tid == 0) a.counts[b] = nk;
    const int ncol = 2 * a.nv;
    for (int r = tid; r < nk; r += 1024) {
        const unsigned long long key = kept_key[r];
        const uint32_t id = decode_order_id(key), s = id / (uint32_t)a.C;
        float *d = a.dets + ((size_t)b * a.max_keep + r) * 5;
        for (int q = 0; q < 4; ++q) d[q] = slotbox[(size_t)s * 4 + q];
        d[4] = decode_order_score(key);
        a.labels[(size_t)b * a.max_keep + r] = (int64_t)(id - s * (uint32_t)a.C);
    }
    for (int e = tid; e < nk * ncol; e += 1024) {
        const int r = e / ncol, i = e - r * ncol;
        const uint32_t s = decode_order_id(kept_key[r]) / (uint32_t)a.C;
        const int l = decode_level_of(a, (int)s);
        const DecodeLv &lv = a.lv[l];
        const int row = lv.select ? a.sel[(size_t)b * a.S + s] : (int)s - lv.slot_off;
        const int y = row / lv.W, x = row - y * lv.W;
        a.vecs[((size_t)b * a.max_keep + r) * ncol + i] =
            decode_vec(decode_map(lv.vec, lv.vs, b), a.kind, i, y, x, decode_geom(a, b, l), slotbox + (size_t)s * 4);
    }
}

// ---- host side ---------------------------------------------------------------------------------
struct DecodePlan {
    int S, keys_per_image, cap2;
    size_t off_maxc, off_keys, off_sel, off_box, off_cand, bytes;
};

static size_t align16(size_t v) { return (v + 15) / 16 * 16; }

// Fills the per-level slot / key offsets of `a` (when given) and the workspace layout; false when a size is out of range.
static bool decode_plan(int B, int L, const lsn_decode_level *levels, int nms_pre, int cand_cap, DecodePlan &p, DecodeArgs *a)
{
    long long S = 0, keys = 0;
    for (int l = 0; l < L; ++l) {
        const long long P = (long long)levels[l].H * levels[l].W;
        if (levels[l].H <= 0 || levels[l].W <= 0 || P > 0x3fffffff) return false;
        const bool select = nms_pre > 0 && nms_pre < P;
        if (a) a->lv[l].select = select, a->lv[l].slot_off = (int)S, a->lv[l].key_off = (int)keys, a->lv[l].K = select ? nms_pre : (int)P;
        S += select ? nms_pre : P;
        keys += select ? P : 0;
        if (S > 0x3fffffff || keys > 0x3fffffff) return false;
    }
    long long cap2 = 1;
    while (cap2 < cand_cap) cap2 <<= 1;
    p.S = (int)S, p.keys_per_image = (int)keys, p.cap2 = (int)cap2;
    size_t o = 0;
    o = align16(o + sizeof(int) * DECODE_MAX_IMAGES), p.off_maxc = o;
    o = align16(o + sizeof(unsigned) * DECODE_MAX_IMAGES), p.off_keys = o;
    o = align16(o + sizeof(unsigned) * (size_t)B * keys), p.off_sel = o;
    o = align16(o + sizeof(int) * (size_t)B * S), p.off_box = o;
    o = align16(o + sizeof(float) * 4 * (size_t)B * S), p.off_cand = o;
    o = align16(o + sizeof(unsigned long long) * (size_t)B * cap2), p.bytes = o;
    return true;
}

static int decode_check_sizes(int B, int L, const lsn_decode_level *levels, int cand_cap)
{
    LSN_CHECK(B >= 1 && B <= DECODE_MAX_IMAGES, "decode: %d images (1..%d)", B, DECODE_MAX_IMAGES);
    LSN_CHECK(L >= 1 && L <= DECODE_MAX_LEVELS, "decode: %d levels (1..%d)", L, DECODE_MAX_LEVELS);
    LSN_CHECK(levels != nullptr, "decode: no levels");
    LSN_CHECK(cand_cap >= 1 && cand_cap <= (1 << 24), "decode: cand_cap %d (1..2^24)", cand_cap);
    return LSN_OK;
}

// Both entry points after their own argument checks.  sources / verify: the corner verification of lsn_decode_cpv_batch (none:
// every level is decoded as it is); num_vectors = 0 and vecs = null: no vector columns.
static int decode_launch(int B, int n_levels, const lsn_decode_level *levels, int n_sources, const lsn_decode_source *sources,
                         const int *verify, int C, const float *img_hw, const float *scale_factors, int num_vectors, int kind,
                         int nms_pre, float score_thr, float iou_thr, int class_agnostic, int max_per_img, int cand_cap, float *dets,
                         float *vecs, int64_t *labels, int32_t *counts, void *workspace, lsn_stream_t stream)
{
    LSN_CHECK(C >= 1, "decode: %d classes", C);
    LSN_CHECK(max_per_img >= 1 && max_per_img <= DECODE_MAX_KEEP, "decode: max_per_img %d (1..%d)", max_per_img, DECODE_MAX_KEEP);
    LSN_CHECK(img_hw && scale_factors && dets && labels && counts && workspace, "decode: null argument");
    static thread_local DecodeArgs A;   // 3.7 KB, passed to the kernels by value
    DecodePlan p;
    LSN_CHECK(decode_plan(B, n_levels, levels, nms_pre, cand_cap, p, &A), "decode: level sizes out of range");
    LSN_CHECK((long long)p.S * C <= 0xffffffffll, "decode: %d slots x %d classes do not fit a 32-bit candidate id", p.S, C);
    for (int l = 0; l < n_levels; ++l) {
        const lsn_decode_level &s = levels[l];
        LSN_CHECK(s.cls && s.box && (s.vec || !vecs), "decode: level %d has a null map", l);
        DecodeLv &d = A.lv[l];
        d.cls = s.cls, d.box = s.box, d.vec = s.vec, d.H = s.H, d.W = s.W, d.stride = s.stride;
        for (int i = 0; i < 4; ++i) d.cs[i] = s.cls_strides[i], d.bs[i] = s.box_strides[i], d.vs[i] = s.vec_strides[i];
        A.verify[l] = verify ? verify[l] : -1;
    }
    for (int k = 0; k < n_sources; ++k) {
        const lsn_decode_source &s = sources[k];
        DecodeSrc &d = A.src[k];
        d.heat = s.heat, d.off = s.offset, d.H = s.H, d.W = s.W, d.stride = s.stride;
        for (int i = 0; i < 4; ++i) d.hs[i] = s.heat_strides[i], d.os[i] = s.offset_strides[i];
    }
    for (int b = 0; b < B; ++b) {
        A.img_hw[b][0] = img_hw[2 * b], A.img_hw[b][1] = img_hw[2 * b + 1];
        for (int i = 0; i < 4; ++i) {
            LSN_CHECK(scale_factors[4 * b + i] > 0.f, "decode: scale factor %d of image %d is not positive", i, b);
            A.sf[b][i] = scale_factors[4 * b + i];
        }
    }
    A.B = B, A.L = n_levels, A.C = C, A.nv = num_vectors, A.kind = kind, A.S = p.S, A.keys_per_image = p.keys_per_image;
    A.cap = cand_cap, A.cap2 = p.cap2, A.max_keep = max_per_img, A.class_agnostic = class_agnostic != 0;
    A.score_thr = score_thr, A.iou_thr = iou_thr;
    char *ws = static_cast<char *>(workspace);
    A.cnt = reinterpret_cast<int *>(ws), A.maxc = reinterpret_cast<unsigned *>(ws + p.off_maxc);
    A.keys = reinterpret_cast<unsigned *>(ws + p.off_keys), A.sel = reinterpret_cast<int *>(ws + p.off_sel);
    A.slotbox = reinterpret_cast<float *>(ws + p.off_box), A.cand = reinterpret_cast<unsigned long long *>(ws + p.off_cand);
    A.dets = dets, A.vecs = vecs, A.labels = labels, A.counts = counts;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double px = 0;      // algorithmic: every logit of a select level read once (candidates and kept rows are a per mille of that)
    for (int l = 0; l < n_levels; ++l) px += A.lv[l].select ? (double)B * levels[l].H * levels[l].W * C : (double)B * A.lv[l].K * C;
    ProfSpan prof(PROF_DECODE, 4.0 * px, 4.0 * px, st);
    hipLaunchKernelGGL(decode_select_kernel, dim3(n_levels, B), dim3(1024), 0, st, A);
    hipLaunchKernelGGL(decode_candidates_kernel, dim3(cdiv(p.S, 256), B), dim3(256), 0, st, A);
    hipLaunchKernelGGL(decode_nms_kernel, dim3(B), dim3(1024), 0, st, A);
    LSN_HIP(hipGetLastError());
    return LSN_OK;
}

}  // namespace lsn

extern "C" {

int64_t lsn_decode_workspace_bytes(int B, int n_levels, const lsn_decode_level *levels, int nms_pre, int cand_cap)
{
    using namespace lsn;
    if (decode_check_sizes(B, n_levels, levels, cand_cap) != LSN_OK) return -1;
    DecodePlan p;
    if (!decode_plan(B, n_levels, levels, nms_pre, cand_cap, p, nullptr)) {
        fail(LSN_ERR_INVALID, "decode: level sizes out of range");
        return -1;
    }
    return (int64_t)p.bytes;
}

int lsn_decode_batch(int B, int n_levels, const lsn_decode_level *levels, int C, const float *img_hw, const float *scale_factors,
                     int num_vectors, int kind, int nms_pre, float score_thr, float iou_thr, int class_agnostic, int max_per_img,
                     int cand_cap, float *dets, float *vecs, int64_t *labels, int32_t *counts, void *workspace, lsn_stream_t stream)
{
    using namespace lsn;
    if (int rc = decode_check_sizes(B, n_levels, levels, cand_cap)) return rc;
    LSN_CHECK(kind == DECODE_BBOX || kind == DECODE_VECTORS || kind == DECODE_POSE_BBOX, "decode: unknown kind %d", kind);
    LSN_CHECK(num_vectors >= 1 && (kind != DECODE_BBOX || num_vectors == 4), "decode: num_vectors %d (kind bbox has 4)", num_vectors);
    LSN_CHECK(vecs, "decode: null argument");
    return decode_launch(B, n_levels, levels, 0, nullptr, nullptr, C, img_hw, scale_factors, num_vectors, kind, nms_pre, score_thr,
                         iou_thr, class_agnostic, max_per_img, cand_cap, dets, vecs, labels, counts, workspace, stream);
}

int lsn_decode_cpv_batch(int B, int n_levels, const lsn_decode_level *levels, int n_sources, const lsn_decode_source *sources,
                         const int *verify_src, int C, const float *img_hw, const float *scale_factors, int nms_pre, float score_thr,
                         float iou_thr, int class_agnostic, int max_per_img, int cand_cap, float *dets, int64_t *labels,
                         int32_t *counts, void *workspace, lsn_stream_t stream)
{
    using namespace lsn;
    if (int rc = decode_check_sizes(B, n_levels, levels, cand_cap)) return rc;
    LSN_CHECK(n_sources >= 0 && n_sources <= DECODE_MAX_SOURCES, "decode: %d corner sources (0..%d)", n_sources, DECODE_MAX_SOURCES);
    LSN_CHECK(verify_src && (sources || n_sources == 0), "decode: null argument");
    for (int s = 0; s < n_sources; ++s) {
        LSN_CHECK(sources[s].H >= 2 && sources[s].W >= 2, "decode: corner source %d is %d x %d (at least 2 x 2)", s, sources[s].H,
                  sources[s].W);
        LSN_CHECK(sources[s].heat && sources[s].offset, "decode: corner source %d has a null map", s);
    }
    for (int l = 0; l < n_levels; ++l)
        LSN_CHECK(verify_src[l] >= -1 && verify_src[l] < n_sources, "decode: level %d verifies against source %d of %d", l,
                  verify_src[l], n_sources);
    return decode_launch(B, n_levels, levels, n_sources, sources, verify_src, C, img_hw, scale_factors, 0, DECODE_BBOX, nms_pre,
                         score_thr, iou_thr, class_agnostic, max_per_img, cand_cap, dets, nullptr, labels, counts, workspace, stream);
}

}  // extern "C"
