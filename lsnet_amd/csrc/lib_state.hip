// lib_state.h: process-wide state with its extern "C" accessors, per-stream device memory.  No kernel, no convolution type.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lib_state.h"
#include "prof.h"

namespace lsn {

static thread_local char g_err[640];
char *err_buf() { return g_err; }
int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// arithmetic of the implicit-GEMM contractions: exact fp32 MFMA, or split-bf16 products (common.h)
static int g_math_mode = -1;   // -1: not initialised (LSNET_MATH decides at first use)
static int math_mode()
{
    if (g_math_mode < 0) {
        const char *e = getenv("LSNET_MATH");
        g_math_mode = (e && (!strcmp(e, "fp32") || !strcmp(e, "exact"))) ? LSN_MATH_FP32
                      : (e && !strcmp(e, "bf16x3"))                       ? LSN_MATH_BF16X3
                      : (e && !strcmp(e, "bf16"))                         ? LSN_MATH_BF16
                                                                          : LSN_MATH_BF16X6;
    }
    return g_math_mode;
}
int math_np()
{
    switch (math_mode()) {
    case LSN_MATH_FP32: return 0;
    case LSN_MATH_BF16: return 1;
    case LSN_MATH_BF16X3: return 3;
    case LSN_MATH_BF16X6: return 6;
    default: return -1;
    }
}

// ---- per-kernel launch timing (prof.h) ----
static const char *const kProfNames[PROF_N] = {"dcn_fwd", "dcn_bwd_data", "dcn_wgrad", "conv_fwd", "conv_bwd_data",
                                               "conv_wgrad", "norm", "gconv", "decode", "points"};
static unsigned g_prof_mask = 0;   // bit f: family f records events
static std::vector<ProfRec> g_prof;
bool prof_on(int fam) { return fam >= 0 && fam < 32 && ((g_prof_mask >> fam) & 1u); }
void prof_push(const ProfRec &r) { g_prof.push_back(r); }
static bool g_launch_log = false;
static std::vector<LaunchRec> g_launches;
bool launch_log_on() { return g_launch_log; }
void launch_log_push(const LaunchRec &r) { g_launches.push_back(r); }

static long long g_stat[4] = {0, 0, 0, 0};
void lib_stat(int which, long long add) { g_stat[which & 3] += add; }

bool stream_capturing(hipStream_t st)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}
int refuse_capture(hipStream_t st, const char *what)
{
    if (!stream_capturing(st)) return 0;
    return fail(LSN_ERR_RUNTIME, "%s inside a stream capture: run the step eagerly once before capturing", what);
}

int device_alloc(void **p, size_t bytes, hipStream_t st, const char *what, bool zero)
{
    if (int rc = refuse_capture(st, what)) return rc;
    LSN_HIP(hipMalloc(p, bytes));
    lib_stat(STAT_MALLOCS, 1), lib_stat(STAT_HELD_BYTES, (long long)bytes);
    if (zero) LSN_HIP(hipMemsetAsync(*p, 0, bytes, st));
    return 0;
}

struct ScratchBlock {
    float *p;
    size_t floats;
};
static PerStream<ScratchBlock> g_scr;
int stream_scratch(size_t floats, float **p, hipStream_t st)
{
    ScratchBlock *sc = nullptr;
    if (int rc = g_scr.get(st, "scratch", &sc, [](ScratchBlock &) { return 0; })) return rc;
    if (floats > sc->floats) {
        const size_t want = floats + floats / 4;
        float *np = nullptr;
        if (int rc = device_alloc(reinterpret_cast<void **>(&np), want * sizeof(float), st, "scratch would grow", false)) return rc;
        sc->p = np, sc->floats = want;   // (the old block stays allocated)
    }
    *p = sc->p;
    return 0;
}

// stream-K arrival counters with the ticket block behind them: one allocation per stream, zeroed once
static PerStream<unsigned *> g_skc;
static int sk_counters(unsigned **p, hipStream_t st)
{
    unsigned **c = nullptr;
    constexpr size_t bytes = (SK_MAX_TILES + LIB_TICKETS) * sizeof(unsigned);
    auto init = [&](unsigned *&np) { return device_alloc(reinterpret_cast<void **>(&np), bytes, st, "scratch would grow", true); };
    if (int rc = g_skc.get(st, "scratch", &c, init)) return rc;
    *p = *c;
    return 0;
}
int stream_sk_scratch(size_t floats, float **part, unsigned **cnt, hipStream_t st)
{
    if (int rc = stream_scratch(floats, part, st)) return rc;
    return sk_counters(cnt, st);
}
int lib_tickets(unsigned **p, hipStream_t st)
{
    const int rc = sk_counters(p, st);
    if (!rc) *p += SK_MAX_TILES;
    return rc;
}

static PerStream<Arena> g_arena;
Arena *arena_of(hipStream_t st) { return g_arena.find(st); }
int arena_get(hipStream_t st, Arena **ar) { return g_arena.get(st, "scratch", ar, [&](Arena &a) { return a.st = st, 0; }); }

// `floats` behind what the arena has handed out.  When it is full the queued reduces run first (`flush`: they consume every
// tile handed out so far, in stream order) and the arena starts over; while it is smaller than the caller's limit
// (lsn_wgrad_defer) it is also replaced by a larger block -- nothing refers to the old one after the flush, so it is freed once
// the stream has drained.  That synchronisation happens only while the arena is still finding its size (the first step at the
// largest shape); in the steady state this function does pointer arithmetic and nothing else.
int arena_alloc(Arena *ar, size_t floats, float **p, int (*flush)(Arena *))
{
    const size_t off = (ar->used + 63) & ~(size_t)63;
    if (off + floats <= ar->floats) {
        *p = ar->p + off;
        ar->used = off + floats;
        return 0;
    }
    if (int rc = flush(ar)) return rc;
    ar->used = 0;
    const size_t limit = (size_t)ar->defer_mb << 18;   // MB -> floats
    if (floats > ar->floats || ar->floats < limit) {
        if (int rc = refuse_capture(ar->st, "scratch would grow")) return rc;
        size_t want = 2 * ar->floats > off + floats ? 2 * ar->floats : off + floats;   // what this step has needed so far, at least doubled
        if (want > limit + floats) want = limit + floats;
        if (want < floats + floats / 4) want = floats + floats / 4;
        want += (size_t)4 << 20;
        if (ar->p) {
            LSN_HIP(hipStreamSynchronize(ar->st));
            lib_stat(STAT_BLOCKING_SYNCS, 1);
            LSN_HIP(hipFree(ar->p));
            lib_stat(STAT_HELD_BYTES, -(long long)(ar->floats * sizeof(float)));
            ar->p = nullptr, ar->floats = 0;
        }
        float *np = nullptr;
        if (hipMalloc(reinterpret_cast<void **>(&np), want * sizeof(float)) != hipSuccess) {
            //  no room for the arena: the queue is empty (flushed above), deferral ends for this stream and
            // the call -- like every later one -- takes the per-stream scratch block with an immediate reduce
            (void)hipGetLastError();
            ar->defer_mb = 0, ar->used = 0;
            return 1;
        }
        lib_stat(STAT_MALLOCS, 1), lib_stat(STAT_HELD_BYTES, (long long)(want * sizeof(float)));
        ar->p = np, ar->floats = want;
    }
    *p = ar->p;
    ar->used = floats;
    return 0;
}

}  // namespace lsn

extern "C" {

const char *lsn_last_error(void) { return lsn::err_buf(); }
int lsn_version(void) { return 100; }

int lsn_set_math_mode(int mode)
{
    LSN_CHECK(mode == LSN_MATH_FP32 || mode == LSN_MATH_BF16X3 || mode == LSN_MATH_BF16X6 || mode == LSN_MATH_BF16,
              "unknown math mode %d", mode);
    lsn::g_math_mode = mode;
    return 0;
}

int lsn_get_math_mode(void) { return lsn::math_mode(); }

int lsn_scratch_stats(long long *out4)
{
    LSN_CHECK(out4 != nullptr, "lsn_scratch_stats: NULL pointer");
    for (int i = 0; i < 4; ++i) out4[i] = lsn::g_stat[i];
    return 0;
}

int lsn_prof_enable(int on)
{
    for (auto &r : lsn::g_prof) {
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    lsn::g_prof.clear();
    lsn::g_prof_mask = on == 1 ? ~0u : (unsigned)on;
    return 0;
}

int lsn_prof_launch_log(int on)
{
    for (auto &r : lsn::g_launches) {
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    lsn::g_launches.clear();
    lsn::g_launch_log = on != 0;
    return 0;
}

int lsn_prof_read_launches(lsn_prof_launch *out, int max_entries)
{
    using namespace lsn;
    const int n = (int)g_launches.size();
    if (out == nullptr) return n;
    int k = 0;
    for (; k < n && k < max_entries; ++k) {
        const LaunchRec &r = g_launches[k];
        LSN_HIP(hipEventSynchronize(r.e1));
        float ms = 0.f;
        LSN_HIP(hipEventElapsedTime(&ms, r.e0, r.e1));
        lsn_prof_launch &o = out[k];
        o.kind = r.v[0], o.C = r.v[1], o.Co = r.v[2], o.kh = r.v[3], o.kw = r.v[4], o.stride = r.v[5], o.pad = r.v[6];
        o.dil = r.v[7], o.relu = r.v[8], o.xpitch = r.v[9], o.n_levels = r.v[10], o.has_residual = r.v[11], o.has_gate = r.v[12];
        for (int i = 0; i < 16; ++i) o.B[i] = r.B[i], o.H[i] = r.H[i], o.W[i] = r.W[i];
        o.ms = ms;
    }
    return k;
}

int lsn_prof_read(lsn_prof_entry *out, int max_entries)
{
    using namespace lsn;
    LSN_CHECK(out != nullptr && max_entries >= PROF_N, "lsn_prof_read needs room for %d entries", PROF_N);
    for (int f = 0; f < PROF_N; ++f) {
        std::memset(&out[f], 0, sizeof(out[f]));
        std::snprintf(out[f].name, sizeof(out[f].name), "%s", kProfNames[f]);
    }
    for (auto &r : g_prof) {
        LSN_HIP(hipEventSynchronize(r.e1));
        float ms = 0.f;
        LSN_HIP(hipEventElapsedTime(&ms, r.e0, r.e1));
        lsn_prof_entry &e = out[r.fam];
        e.launches += 1;
        e.total_ms += ms;
        e.flops += r.flops;
        e.bytes += r.bytes;
    }
    return PROF_N;
}

}  // extern "C"
