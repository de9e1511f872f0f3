// Corner-point verification of liblsnet_hip.so: the heat-map / offset targets of PointHMAssigner and the three losses
// LSCPVHead adds to LSHead (corner heat-map, corner offset, box-level semantics).
#include "common.h"
#include "cpv_rows.h"

namespace lsn {

// ---------------------------------------------------------------------------------------------
// Streaming and reduction kernels, no matrix work.  What they are built for: few launches (2 for the targets of a batch, 2
// for a loss forward over all levels, 1 for a backward), one pass over the maps, and a FIXED summation order -- every
// workgroup reduces its elements in lane / wave order into its own slot, a finishing workgroup adds the slots in index
// order.  The slots and their sums are doubles: the result is the fp32 element values added (nearly) exactly.  No atomics.
// ---------------------------------------------------------------------------------------------
constexpr int CPV_MAX_IMAGES = 64;
constexpr int CPV_MAX_LEVELS = 8;
constexpr int CPV_THREADS = 256;

struct CpvBatch {
    int B;
    int off[CPV_MAX_IMAGES + 1];   // gt rows of image b: [off[b], off[b + 1])
};

// sum of v over the workgroup's CPV_THREADS threads, in lane then wave order; the value is returned to every thread
__device__ __forceinline__ double block_sum(double v, double *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int tid = threadIdx.x;
    __syncthreads();                                     // (red may still be read from an earlier call)
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < CPV_THREADS / 64; ++w) s += red[w];
    return s;
}

// ---- targets -----------------------------------------------------------------------------------
// workspace: int win[G * 2 * CPV_LEVELS] (the point row a gt's corner takes on a level, -1: none) | float rs[G * 2] (radius, sigma)

// one workgroup per (gt, corner, level): the nearest valid point of the level, equal distances to the lowest row
__global__ __launch_bounds__(CPV_THREADS) void corner_nearest_kernel(const float *__restrict__ points, int P,
                                                                     const uint8_t *__restrict__ valid,
                                                                     const float *__restrict__ gt, CpvBatch bt, int bump,
                                                                     cpv_radius_consts rk, int *__restrict__ win,
                                                                     float *__restrict__ rs)
{
    __shared__ unsigned long long red[CPV_THREADS / 64];
    const int g = blockIdx.x >> 1, c = blockIdx.x & 1, lev = blockIdx.y, tid = threadIdx.x;
    int b = 0;
    while (b + 1 < bt.B && g >= bt.off[b + 1]) ++b;
    const float *box = gt + (size_t)g * 4;
    const float cx = box[2 * c], cy = box[2 * c + 1];
    if (c == 0 && lev == 0 && tid == 0) {
        float r = 0.f, s = 1.f;
        if (bump) {
            r = cpv_gaussian_radius(box[3] - box[1], box[2] - box[0], rk);
            s = cpv_sigma(r);
        }
        rs[(size_t)g * 2] = r, rs[(size_t)g * 2 + 1] = s;
    }
    const uint8_t *vb = valid ? valid + (size_t)b * P : nullptr;
    unsigned long long best = ~0ull;
    for (int i = tid; i < P; i += CPV_THREADS) {
        if (vb && !vb[i]) continue;
        const float *pt = points + (size_t)i * 3;
        if (assign_point_level(pt[2]) != lev) continue;
        const unsigned key = assign_key(cpv_corner_distance(pt[0], pt[1], cx, cy));
        if (key >= 0xff800000u) continue;                 // +inf or NaN distance: the statement's isfinite() sends it to the sink
        const unsigned long long cand = ((unsigned long long)key << 32) | (unsigned)i;
        best = cand < best ? cand : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(best, o);
        best = t < best ? t : best;
    }
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < CPV_THREADS / 64; ++w) best = red[w] < best ? red[w] : best;
        win[((size_t)g * 2 + c) * CPV_LEVELS + lev] = best == ~0ull ? -1 : (int)(best & 0xffffffffu);
    }
}

// one thread per (image, corner, point): Gaussian maximum over the image's gts, the winning gt from the table; the first
// workgroup of every (image, corner) also counts the positives = the distinct point rows of the table
__global__ __launch_bounds__(CPV_THREADS) void corner_write_kernel(const float *__restrict__ points, int P,
                                                                   const uint8_t *__restrict__ valid,
                                                                   const float *__restrict__ gt, CpvBatch bt, int bump,
                                                                   const int *__restrict__ win, const float *__restrict__ rs,
                                                                   float *__restrict__ hm, float *__restrict__ off,
                                                                   int *__restrict__ npos)
{
    __shared__ int cnt[CPV_THREADS / 64];
    const int c = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int g0 = bt.off[b], g1 = bt.off[b + 1];
    const int p = blockIdx.x * CPV_THREADS + tid;
    if (p < P) {
        const size_t o = ((size_t)b * 2 + c) * P + p;
        float h = 0.f, ox = 0.f, oy = 0.f;
        if (!valid || valid[(size_t)b * P + p]) {
            const float px = points[(size_t)p * 3], py = points[(size_t)p * 3 + 1];
            const int lev = assign_point_level(points[(size_t)p * 3 + 2]);
            const bool on = lev >= 0 && lev < CPV_LEVELS;
            int winner = -1;
            for (int g = g0; g < g1; ++g) {
                if (bump) {
                    const float cx = gt[(size_t)g * 4 + 2 * c], cy = gt[(size_t)g * 4 + 2 * c + 1];
                    h = fmaxf(h, cpv_heat(cpv_corner_distance(px, py, cx, cy), rs[(size_t)g * 2], rs[(size_t)g * 2 + 1]));
                }
                if (on && win[((size_t)g * 2 + c) * CPV_LEVELS + lev] == p) winner = g;      // the last gt keeps a shared point
            }
            if (winner >= 0) {
                h = 1.f;
                ox = cpv_offset(gt[(size_t)winner * 4 + 2 * c], px, lev);
                oy = cpv_offset(gt[(size_t)winner * 4 + 2 * c + 1], py, lev);
            }
        }
        hm[o] = h;
        off[o * 2] = ox, off[o * 2 + 1] = oy;
    }
    if (blockIdx.x != 0) return;
    int n = 0;
    const int entries = (g1 - g0) * CPV_LEVELS;
    for (int e = tid; e < entries; e += CPV_THREADS) {
        const int g = g0 + e / CPV_LEVELS, lev = e % CPV_LEVELS;
        const int row = win[((size_t)g * 2 + c) * CPV_LEVELS + lev];
        if (row < 0) continue;
        bool later = false;
        for (int q = g + 1; q < g1 && !later; ++q) later = win[((size_t)q * 2 + c) * CPV_LEVELS + lev] == row;
        n += later ? 0 : 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((tid & 63) == 0) cnt[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < CPV_THREADS / 64; ++w) n += cnt[w];
        npos[b * 2 + c] = n;
    }
}

// ---- corner losses -----------------------------------------------------------------------------
struct CornerLevel {
    int H, W, pstart, blk_start;
    const float *score, *offset;
    float *gscore, *goffset;
    int64_t ss[4], os[4], gss[4], gos[4];
};
struct CornerLevels {
    int n, B, P, blocks;
    CornerLevel lv[CPV_MAX_LEVELS];
};

__device__ __forceinline__ int level_of_block(const CornerLevels &L, int blk)
{
    int l = 0;
    while (l + 1 < L.n && blk >= L.lv[l + 1].blk_start) ++l;
    return l;
}

// n_c = sum_b max(npos[b, c], 1), as a float (the head's avg_factor)
__device__ __forceinline__ float corner_count(const int *__restrict__ npos, int B, int c)
{
    int n = 0;
    for (int b = 0; b < B; ++b) n += npos[b * 2 + c] > 1 ? npos[b * 2 + c] : 1;
    return (float)n;
}

// one thread per (image, cell) of a level, both corners.  BWD = false: the workgroup's four sums (heat tl, heat br, offset tl,
// offset br) to partial[block * 4 ..]; BWD = true: the gradients of the cell's 2 + 4 map values.
template <bool BWD>
__global__ __launch_bounds__(CPV_THREADS) void corner_loss_kernel(CornerLevels L, const float *__restrict__ hm,
                                                                  const float *__restrict__ off,
                                                                  const uint8_t *__restrict__ valid,
                                                                  const int *__restrict__ npos, float alpha, float gamma,
                                                                  float beta, double *__restrict__ partial,
                                                                  const float *__restrict__ g_heat,
                                                                  const float *__restrict__ g_off)
{
    __shared__ double red[CPV_THREADS / 64];
    const int l = level_of_block(L, blockIdx.x);
    const CornerLevel &lv = L.lv[l];
    const int hw = lv.H * lv.W;
    const long long idx = (long long)(blockIdx.x - lv.blk_start) * CPV_THREADS + threadIdx.x;
    const bool live = idx < (long long)L.B * hw;
    double sum[4] = {0., 0., 0., 0.};
    float gh[2] = {0.f, 0.f}, go[2] = {0.f, 0.f};
    if (BWD) {
        for (int c = 0; c < 2; ++c) {
            const float n = corner_count(npos, L.B, c);
            gh[c] = g_heat[l] / 2.f / n, go[c] = g_off[l] / 2.f / n;
        }
    }
    if (live) {
        const int b = (int)(idx / hw), cell = (int)(idx - (long long)b * hw), y = cell / lv.W, x = cell - y * lv.W;
        const int p = lv.pstart + cell;
        const bool v = !valid || valid[(size_t)b * L.P + p];
        for (int c = 0; c < 2; ++c) {
            const size_t o = ((size_t)b * 2 + c) * L.P + p;
            const float t = hm[o];
            const int64_t si = b * lv.ss[0] + c * lv.ss[1] + y * lv.ss[2] + x * lv.ss[3];
            float dx = 0.f;
            const float val = cpv_gaussian_focal(lv.score[si], t, alpha, gamma, BWD ? &dx : nullptr);
            if (BWD)
                lv.gscore[b * lv.gss[0] + c * lv.gss[1] + y * lv.gss[2] + x * lv.gss[3]] = v ? gh[c] * dx : 0.f;
            else if (v)
                sum[c] += (double)val;
            for (int k = 0; k < 2; ++k) {
                const int64_t oi = b * lv.os[0] + (2 * c + k) * lv.os[1] + y * lv.os[2] + x * lv.os[3];
                const bool pos = v && t == 1.f;
                float dp = 0.f;
                const float sl = pos ? cpv_smooth_l1(lv.offset[oi], off[o * 2 + k], beta, BWD ? &dp : nullptr) : 0.f;
                if (BWD)
                    lv.goffset[b * lv.gos[0] + (2 * c + k) * lv.gos[1] + y * lv.gos[2] + x * lv.gos[3]] = pos ? go[c] * dp : 0.f;
                else
                    sum[2 + c] += (double)sl;
            }
        }
    }
    if (!BWD) {
        for (int j = 0; j < 4; ++j) {
            const double s = block_sum(sum[j], red);
            if (threadIdx.x == 0) partial[(size_t)blockIdx.x * 4 + j] = s;
        }
    }
}

// one workgroup per level: its slots in index order -> the two normalised losses
__global__ __launch_bounds__(CPV_THREADS) void corner_loss_finish_kernel(CornerLevels L, const double *__restrict__ partial,
                                                                         const int *__restrict__ npos,
                                                                         float *__restrict__ loss_heat,
                                                                         float *__restrict__ loss_off)
{
    __shared__ double red[CPV_THREADS / 64];
    const int l = blockIdx.x;
    const int b0 = L.lv[l].blk_start, b1 = l + 1 < L.n ? L.lv[l + 1].blk_start : L.blocks;
    double s[4];
    for (int j = 0; j < 4; ++j) {
        double a = 0.;
        for (int k = b0 + threadIdx.x; k < b1; k += CPV_THREADS) a += partial[(size_t)k * 4 + j];
        s[j] = block_sum(a, red);
    }
    if (threadIdx.x == 0) {
        const float n0 = corner_count(npos, L.B, 0), n1 = corner_count(npos, L.B, 1);
        loss_heat[l] = ((float)s[0] / n0 + (float)s[1] / n1) / 2.f;
        loss_off[l] = ((float)s[2] / n0 + (float)s[3] / n1) / 2.f;
    }
}

// ---- semantic (SEP focal) loss -------------------------------------------------------------------
struct SemLevel {
    int H, W, blk_start, nhwc;
    const float *logits;
    float *grad;
    int64_t st[4], gst[4];
};
struct SemLevels {
    int n, B, C, h, w, blocks;
    SemLevel lv[CPV_MAX_LEVELS];
};
constexpr int SEM_PER_THREAD = 4;

// CPV_THREADS * SEM_PER_THREAD elements per workgroup, walked in the order of the level's memory format.  BWD = false: the
// five sums (positive loss, positive weights, negative loss, count target == 1, count target > 0) to partial[block * 5 ..].
template <bool BWD>
__global__ __launch_bounds__(CPV_THREADS) void sep_focal_kernel(SemLevels L, const float *__restrict__ target,
                                                                const float *__restrict__ weight, float gamma, float alpha,
                                                                double *__restrict__ partial, const float *__restrict__ stats,
                                                                const float *__restrict__ g)
{
    __shared__ double red[CPV_THREADS / 64];
    int l = 0;
    while (l + 1 < L.n && (int)blockIdx.x >= L.lv[l + 1].blk_start) ++l;
    const SemLevel &lv = L.lv[l];
    const long long total = (long long)L.B * L.C * lv.H * lv.W;
    double sum[5] = {0., 0., 0., 0., 0.};
    float gpos = 0.f, gneg = 0.f;
    if (BWD) {
        gpos = stats[1] != 0.f ? g[0] / stats[0] : 0.f;      // d(pos_loss / wsum); no positives: the term is the constant 0
        gneg = g[0] / stats[2];                               // d(neg_loss / count(target > 0))
    }
    for (int j = 0; j < SEM_PER_THREAD; ++j) {
        const long long idx = ((long long)(blockIdx.x - lv.blk_start) * SEM_PER_THREAD + j) * CPV_THREADS + threadIdx.x;
        if (idx >= total) break;
        int b, c, y, x;
        long long r = idx;
        if (lv.nhwc) {
            c = (int)(r % L.C), r /= L.C;
            x = (int)(r % lv.W), r /= lv.W;
            y = (int)(r % lv.H), b = (int)(r / lv.H);
        } else {
            x = (int)(r % lv.W), r /= lv.W;
            y = (int)(r % lv.H), r /= lv.H;
            c = (int)(r % L.C), b = (int)(r / L.C);
        }
        const size_t ti = (((size_t)b * L.C + c) * L.h + cpv_nearest_index(y, L.h, lv.H)) * L.w + cpv_nearest_index(x, L.w, lv.W);
        const float t = target[ti];
        const int64_t li = b * lv.st[0] + c * lv.st[1] + y * lv.st[2] + x * lv.st[3];
        const float xv = lv.logits[li];
        float d = 0.f, grad = 0.f;
        if (t == 1.f) {
            const float wv = weight[ti];
            const float v = cpv_sep_focal_pos(xv, wv, gamma, alpha, BWD ? &d : nullptr);
            sum[0] += (double)v, sum[1] += (double)wv, sum[3] += 1.;
            grad = gpos * d;
        } else if (t < 1.f) {
            const float v = cpv_sep_focal_neg(xv, gamma, alpha, BWD ? &d : nullptr);
            sum[2] += (double)v;
            grad = gneg * d;
        }
        if (t > 0.f) sum[4] += 1.;
        if (BWD) lv.grad[b * lv.gst[0] + c * lv.gst[1] + y * lv.gst[2] + x * lv.gst[3]] = grad;
    }
    if (!BWD) {
        for (int j = 0; j < 5; ++j) {
            const double s = block_sum(sum[j], red);
            if (threadIdx.x == 0) partial[(size_t)blockIdx.x * 5 + j] = s;
        }
    }
}

// one workgroup: all slots in index order -> the loss and what backward needs
__global__ __launch_bounds__(CPV_THREADS) void sep_focal_finish_kernel(int blocks, const double *__restrict__ partial,
                                                                       float *__restrict__ loss, float *__restrict__ stats)
{
    __shared__ double red[CPV_THREADS / 64];
    double s[5];
    for (int j = 0; j < 5; ++j) {
        double a = 0.;
        for (int k = threadIdx.x; k < blocks; k += CPV_THREADS) a += partial[(size_t)k * 5 + j];
        s[j] = block_sum(a, red);
    }
    if (threadIdx.x == 0) {
        const float pos_loss = (float)s[0], wsum = (float)s[1], neg_loss = (float)s[2], avg = (float)s[4];
        const float pos_term = s[3] > 0. ? pos_loss / wsum : 0.f;
        loss[0] = pos_term + neg_loss / avg;
        stats[0] = wsum, stats[1] = s[3] > 0. ? 1.f : 0.f, stats[2] = avg, stats[3] = (float)s[3];
    }
}

static int make_batch(CpvBatch &bt, int B, const int *gt_offset, const char *what)
{
    LSN_CHECK(B >= 1 && B <= CPV_MAX_IMAGES, "%s: %d images (1 .. %d)", what, B, CPV_MAX_IMAGES);
    LSN_CHECK(gt_offset && gt_offset[0] == 0, "%s: gt_offset must start at 0", what);
    bt.B = B;
    for (int b = 0; b <= B; ++b) {
        LSN_CHECK(b == 0 || gt_offset[b] >= gt_offset[b - 1], "%s: gt_offset must not decrease", what);
        bt.off[b] = gt_offset[b];
    }
    return 0;
}

static int make_corner_levels(CornerLevels &L, int B, int P, int n_levels, const lsn_corner_level *levels, bool backward,
                              const char *what)
{
    LSN_CHECK(B >= 1 && B <= CPV_MAX_IMAGES, "%s: %d images (1 .. %d)", what, B, CPV_MAX_IMAGES);
    LSN_CHECK(n_levels >= 1 && n_levels <= CPV_MAX_LEVELS && levels, "%s: %d levels (1 .. %d)", what, n_levels, CPV_MAX_LEVELS);
    L.n = n_levels, L.B = B, L.P = P;
    long long pstart = 0, blk = 0;
    for (int l = 0; l < n_levels; ++l) {
        const lsn_corner_level &s = levels[l];
        LSN_CHECK(s.H > 0 && s.W > 0 && (long long)B * s.H * s.W < (1ll << 31), "%s: level %d is %d x %d", what, l, s.H, s.W);
        LSN_CHECK(s.score && s.offset, "%s: level %d has a NULL map", what, l);
        LSN_CHECK(!backward || (s.grad_score && s.grad_offset), "%s: level %d has a NULL gradient map", what, l);
        CornerLevel &d = L.lv[l];
        d.H = s.H, d.W = s.W, d.pstart = (int)pstart, d.blk_start = (int)blk;
        d.score = s.score, d.offset = s.offset, d.gscore = s.grad_score, d.goffset = s.grad_offset;
        for (int k = 0; k < 4; ++k) {
            LSN_CHECK(s.score_strides[k] >= 0 && s.offset_strides[k] >= 0, "%s: level %d has a negative stride", what, l);
            d.ss[k] = s.score_strides[k], d.os[k] = s.offset_strides[k];
            LSN_CHECK(!backward || (s.grad_score_strides[k] >= 0 && s.grad_offset_strides[k] >= 0),
                      "%s: level %d has a negative gradient stride", what, l);
            d.gss[k] = backward ? s.grad_score_strides[k] : 0, d.gos[k] = backward ? s.grad_offset_strides[k] : 0;
        }
        pstart += (long long)s.H * s.W;
        blk += ((long long)B * s.H * s.W + CPV_THREADS - 1) / CPV_THREADS;
        LSN_CHECK(pstart < (1ll << 31) && blk < (1ll << 31), "%s: the levels are too large", what);
    }
    LSN_CHECK(pstart == P, "%s: the levels hold %lld points, P = %d", what, pstart, P);
    LSN_CHECK((long long)B * 2 * P < (1ll << 31), "%s: %d x %d points", what, B, P);
    L.blocks = (int)blk;
    return 0;
}

static int make_sem_levels(SemLevels &L, int B, int C, int n_levels, const lsn_sem_level *levels, int h, int w, bool backward,
                           const char *what)
{
    LSN_CHECK(B >= 1 && C >= 1 && h >= 1 && w >= 1, "%s: B = %d, C = %d, target maps %d x %d", what, B, C, h, w);
    LSN_CHECK((long long)B * C * h * w < (1ll << 31), "%s: target maps of %d x %d x %d x %d", what, B, C, h, w);
    LSN_CHECK(n_levels >= 1 && n_levels <= CPV_MAX_LEVELS && levels, "%s: %d levels (1 .. %d)", what, n_levels, CPV_MAX_LEVELS);
    L.n = n_levels, L.B = B, L.C = C, L.h = h, L.w = w;
    long long blk = 0;
    const long long per = (long long)CPV_THREADS * SEM_PER_THREAD;
    for (int l = 0; l < n_levels; ++l) {
        const lsn_sem_level &s = levels[l];
        LSN_CHECK(s.H > 0 && s.W > 0 && (long long)B * C * s.H * s.W < (1ll << 40), "%s: level %d is %d x %d", what, l, s.H, s.W);
        LSN_CHECK(s.logits && (!backward || s.grad), "%s: level %d has a NULL map", what, l);
        SemLevel &d = L.lv[l];
        d.H = s.H, d.W = s.W, d.blk_start = (int)blk, d.logits = s.logits, d.grad = s.grad;
        for (int k = 0; k < 4; ++k) {
            LSN_CHECK(s.strides[k] >= 0, "%s: level %d has a negative stride", what, l);
            LSN_CHECK(!backward || s.grad_strides[k] >= 0, "%s: level %d has a negative gradient stride", what, l);
            d.st[k] = s.strides[k], d.gst[k] = backward ? s.grad_strides[k] : 0;
        }
        d.nhwc = C > 1 && s.strides[1] == 1;
        blk += ((long long)B * C * s.H * s.W + per - 1) / per;
        LSN_CHECK(blk < (1ll << 31), "%s: the levels are too large", what);
    }
    L.blocks = (int)blk;
    return 0;
}

}  // namespace lsn

using namespace lsn;

int64_t lsn_corner_targets_workspace_bytes(int G)
{
    if (G < 0) return 0;
    return 64 + (int64_t)G * (2 * CPV_LEVELS * 4 + 8);
}

int lsn_corner_targets_batch(const float *points, int P, const uint8_t *valid, const float *gt_bboxes, int B,
                             const int *gt_offset, int gaussian_bump, double gaussian_iou, float *hm, float *off,
                             int32_t *npos, void *workspace, lsn_stream_t stream)
{
    CpvBatch bt;
    if (int rc = make_batch(bt, B, gt_offset, "corner targets")) return rc;
    const int G = bt.off[B];
    LSN_CHECK(P > 0 && G > 0, "corner targets: P = %d, G = %d (empty inputs are the caller's)", P, G);
    LSN_CHECK(G < (1 << 24), "corner targets: %d gts", G);
    LSN_CHECK(!gaussian_bump || (gaussian_iou > 0. && gaussian_iou < 1.), "corner targets: gaussian_iou %g", gaussian_iou);
    LSN_CHECK(points && gt_bboxes && hm && off && npos && workspace, "corner targets: NULL argument");
    LSN_CHECK((long long)B * 2 * P < (1ll << 30), "corner targets: %d x %d points", B, P);
    int *win = static_cast<int *>(workspace);
    float *rs = reinterpret_cast<float *>(win + (size_t)G * 2 * CPV_LEVELS);
    const cpv_radius_consts rk = cpv_radius_constants(gaussian_iou);
    hipLaunchKernelGGL(corner_nearest_kernel, dim3(G * 2, CPV_LEVELS), dim3(CPV_THREADS), 0, stream, points, P, valid, gt_bboxes,
                       bt, gaussian_bump, rk, win, rs);
    hipLaunchKernelGGL(corner_write_kernel, dim3(cdiv(P, CPV_THREADS), 2, B), dim3(CPV_THREADS), 0, stream, points, P, valid,
                       gt_bboxes, bt, gaussian_bump, win, rs, hm, off, npos);
    LSN_HIP(hipGetLastError());
    return 0;
}

int64_t lsn_corner_loss_workspace_bytes(int B, int n_levels, const lsn_corner_level *levels)
{
    if (B < 1 || n_levels < 1 || n_levels > CPV_MAX_LEVELS || !levels) return 0;
    int64_t blk = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (levels[l].H <= 0 || levels[l].W <= 0) return 0;
        blk += ((int64_t)B * levels[l].H * levels[l].W + CPV_THREADS - 1) / CPV_THREADS;
    }
    return 64 + blk * 4 * 8;
}

int lsn_corner_loss_forward(int B, int P, int n_levels, const lsn_corner_level *levels, const float *hm, const float *off,
                            const uint8_t *valid, const int32_t *npos, float alpha, float gamma, float beta,
                            float *loss_heat, float *loss_off, void *workspace, lsn_stream_t stream)
{
    CornerLevels L;
    if (int rc = make_corner_levels(L, B, P, n_levels, levels, false, "corner loss")) return rc;
    LSN_CHECK(beta > 0.f, "corner loss: beta %g", (double)beta);
    LSN_CHECK(hm && off && npos && loss_heat && loss_off && workspace, "corner loss: NULL argument");
    LSN_CHECK((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "corner loss: workspace must be 8-byte aligned");
    double *partial = static_cast<double *>(workspace);
    hipLaunchKernelGGL(corner_loss_kernel<false>, dim3(L.blocks), dim3(CPV_THREADS), 0, stream, L, hm, off, valid, npos, alpha,
                       gamma, beta, partial, static_cast<const float *>(nullptr), static_cast<const float *>(nullptr));
    hipLaunchKernelGGL(corner_loss_finish_kernel, dim3(L.n), dim3(CPV_THREADS), 0, stream, L, partial, npos, loss_heat, loss_off);
    LSN_HIP(hipGetLastError());
    return 0;
}

int lsn_corner_loss_backward(int B, int P, int n_levels, const lsn_corner_level *levels, const float *hm, const float *off,
                             const uint8_t *valid, const int32_t *npos, float alpha, float gamma, float beta,
                             const float *g_heat, const float *g_off, lsn_stream_t stream)
{
    CornerLevels L;
    if (int rc = make_corner_levels(L, B, P, n_levels, levels, true, "corner loss backward")) return rc;
    LSN_CHECK(beta > 0.f, "corner loss backward: beta %g", (double)beta);
    LSN_CHECK(hm && off && npos && g_heat && g_off, "corner loss backward: NULL argument");
    hipLaunchKernelGGL(corner_loss_kernel<true>, dim3(L.blocks), dim3(CPV_THREADS), 0, stream, L, hm, off, valid, npos, alpha,
                       gamma, beta, static_cast<double *>(nullptr), g_heat, g_off);
    LSN_HIP(hipGetLastError());
    return 0;
}

int64_t lsn_sep_focal_workspace_bytes(int B, int C, int n_levels, const lsn_sem_level *levels)
{
    if (B < 1 || C < 1 || n_levels < 1 || n_levels > CPV_MAX_LEVELS || !levels) return 0;
    const int64_t per = (int64_t)CPV_THREADS * SEM_PER_THREAD;
    int64_t blk = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (levels[l].H <= 0 || levels[l].W <= 0) return 0;
        blk += ((int64_t)B * C * levels[l].H * levels[l].W + per - 1) / per;
    }
    return 64 + blk * 5 * 8;
}

int lsn_sep_focal_forward(int B, int C, int n_levels, const lsn_sem_level *levels, const float *target, const float *weight,
                          int h, int w, float gamma, float alpha, float *loss, float *stats, void *workspace,
                          lsn_stream_t stream)
{
    SemLevels L;
    if (int rc = make_sem_levels(L, B, C, n_levels, levels, h, w, false, "sep focal")) return rc;
    LSN_CHECK(target && weight && loss && stats && workspace, "sep focal: NULL argument");
    LSN_CHECK((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "sep focal: workspace must be 8-byte aligned");
    double *partial = static_cast<double *>(workspace);
    hipLaunchKernelGGL(sep_focal_kernel<false>, dim3(L.blocks), dim3(CPV_THREADS), 0, stream, L, target, weight, gamma, alpha,
                       partial, static_cast<const float *>(nullptr), static_cast<const float *>(nullptr));
    hipLaunchKernelGGL(sep_focal_finish_kernel, dim3(1), dim3(CPV_THREADS), 0, stream, L.blocks, partial, loss, stats);
    LSN_HIP(hipGetLastError());
    return 0;
}

int lsn_sep_focal_backward(int B, int C, int n_levels, const lsn_sem_level *levels, const float *target, const float *weight,
                           int h, int w, float gamma, float alpha, const float *stats, const float *g, lsn_stream_t stream)
{
    SemLevels L;
    if (int rc = make_sem_levels(L, B, C, n_levels, levels, h, w, true, "sep focal backward")) return rc;
    LSN_CHECK(target && weight && stats && g, "sep focal backward: NULL argument");
    hipLaunchKernelGGL(sep_focal_kernel<true>, dim3(L.blocks), dim3(CPV_THREADS), 0, stream, L, target, weight, gamma, alpha,
                       static_cast<double *>(nullptr), stats, g);
    LSN_HIP(hipGetLastError());
    return 0;
}
