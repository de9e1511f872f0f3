// The library's shared host side.  lib_state.hip owns the process-wide state (error text, math mode, profiler storage: prof.h,
// the lsn_scratch_stats counters) and the device memory the library keeps per stream.  A function that one .hip file defines
// and another calls is declared HERE (or in prof.h / common.h) and nowhere else, and the defining file includes this header:
// a changed parameter list is a compile error, not a link that misbehaves.
#pragma once
#include <vector>

#include "common.h"
#include "conv_wgrad_route.h"
#include "per_stream.h"

namespace lsn {

// lsn_scratch_stats counters: what the library itself asks of the HIP runtime outside launches -- a training loop whose shapes
// change every iteration (multi-scale training) must reach a state in which none of these moves any more
enum { STAT_MALLOCS = 0, STAT_HELD_BYTES = 1, STAT_BLOCKING_SYNCS = 2, STAT_POOL_ALLOCS = 3 };
void lib_stat(int which, long long add);

// bf16 products per fp32 product of the current math mode (0: exact fp32 MFMA; -1: unknown, which split_dispatch refuses)
int math_np();

bool stream_capturing(hipStream_t st);
// 0, or LSN_ERR_RUNTIME "<what> inside a stream capture: run the step eagerly once before capturing" while st is being captured
int refuse_capture(hipStream_t st, const char *what);
// refuse_capture(st, what), hipMalloc, the counters, with `zero` a fill in stream order.  Never freed: a graph may hold it.
int device_alloc(void **p, size_t bytes, hipStream_t st, const char *what, bool zero);

// ---- per stream: callers on different streams share none of these.  Host-side bookkeeping, not thread-safe. ----
// The scratch block for the partial results of split reductions, valid until the stream's next request.  An outgrown block is
// RETIRED, not freed; growing under capture is refused -- run the step eagerly once first (the graph wrapper's warm-ups do).
int stream_scratch(size_t floats, float **p, hipStream_t st);
// scratch + the arrival counters of stream-K tiles: SK_MAX_TILES of them, zeroed once, every launch leaves them zero
constexpr int SK_MAX_TILES = 4096;
int stream_sk_scratch(size_t floats, float **part, unsigned **cnt, hipStream_t st);
// LIB_TICKETS tickets of last-arriver reductions behind those counters: a kernel finds its slot zero and leaves it zero
constexpr int LIB_TICKETS = 1024;
enum { TICKET_FOCAL_SUM = 0, TICKET_GN_IMGSUM = 1 };
int lib_tickets(unsigned **p, hipStream_t st);

// Memory of the deferred weight-gradient reduces (lsn_wgrad_defer): partial tiles that stay untouched until conv.hip, which owns
// the queue, has run the reduces that read them.  RJob: one queued reduce -- carried here, never looked into.
struct RJob;
struct Arena {
    hipStream_t st;
    float *p;
    size_t floats, used;
    long long defer_mb;   // 0: off
    std::vector<RJob> *jobs;
};
Arena *arena_of(hipStream_t st);             // nullptr: the stream never asked for deferral
int arena_get(hipStream_t st, Arena **ar);   // ... created when it is not there
// `floats` of arena space; `flush` runs the owner's queued reduces when the arena has to start over.  1: no memory for the
// arena -- deferral is off for the stream from now on, the caller takes the scratch block
int arena_alloc(Arena *ar, size_t floats, float **p, int (*flush)(Arena *));

// One validated weight-gradient call of a dense convolution (conv.hip conv_wgrad_call builds it, conv_wgrad_route.h routes it)
struct WgFoldJobs;   // the folded BatchNorm(s) of the call (conv_wgrad_kernels.h) -- carried here, never looked into
struct ConvWgradCall {
    ConvWgradShape s;   // levels with Ho, Wo and pixel counts; C, Co, kh, kw, stride, dil; what else the route looks at
    const float *x[CW_MAXLV], *go[CW_MAXLV];
    int pad, accumulate;
    float *gw, *gb;
    const WgFoldJobs *fold;   // nullptr: a plain call
};

// ---- conv.hip, for dcn.hip ----
// partial tiles of ONE weight-gradient call: from the arena while the stream defers, else the scratch block
int wgrad_part_buffer(size_t floats, float **p, hipStream_t st);
int conv_mm_rows(int n, const float *const *x, float *const *out, const int *rows, int Cr, int xpitch, int N,
                 const unsigned short *wf, hipStream_t st);
// gw (+)= sum of `splits` partial gradients of n floats (n % 4 == 0), gb (+)= sum of splits_b partial rows of nb; launched, or
// queued while the stream defers.  fold: the reduce also applies the norm's scale and forms grad_gamma / grad_beta
int conv_wgrad_reduce(const float *part, float *gw, size_t n, const float *part_b, float *gb, int nb, int splits, int splits_b,
                      int accumulate, const WgFoldJobs *fold, hipStream_t st);

// ---- dcn.hip, for conv.hip: the two routes of a dense weight gradient on the deformable family's kernels ----
bool general_gemms_only();   // LSN_DBG_GENERAL_GEMMS is set
int conv_wgrad_dense_mm(const ConvWgradCall &c, hipStream_t st);   // CW_DENSE_MM: the fragment-order kernel with the tap table
// CW_GENERAL: the PLAIN split kernel with its ordered reduce (fp32 atomics above 256 MB of partial tiles; refused under a fold)
int conv_wgrad_general(const ConvWgradCall &c, hipStream_t st);

}  // namespace lsn
