// One table per kind of state the library keeps per stream: at most 16 streams, a linear search, an entry created by the first
// call that needs it.  Entries never move (callers and captured graphs hold pointers into them) and are never removed.
// No HIP here: the key is the stream handle as an opaque pointer, so the table compiles -- and is tested -- on the host alone.
// It needs lsn::fail (common.h) declared before this header is included: lib_state.h does that, a host test supplies its own.
#pragma once
#include "../../include/lsnet_hip.h"

namespace lsn {

template <class T> class PerStream {
public:
    static constexpr int CAP = 16;

    // the stream's entry, or nullptr; creates nothing
    T *find(const void *stream)
    {
        for (int i = 0; i < n_; ++i)
            if (key_[i] == stream) return &val_[i];
        return nullptr;
    }

    // *out = the stream's entry, created by init(T &) -> int (0, or the error it returns: the slot stays free then)
    template <class Init> int get(const void *stream, const char *name, T **out, Init &&init)
    {
        if ((*out = find(stream))) return 0;
        if (n_ == CAP) return fail(LSN_ERR_RUNTIME, "%s: more than %d streams use the library", name, CAP);
        val_[n_] = T();
        if (int rc = init(val_[n_])) return rc;
        key_[n_] = stream;
        *out = &val_[n_++];
        return 0;
    }

private:
    const void *key_[CAP] = {};
    T val_[CAP] = {};
    int n_ = 0;
};

}  // namespace lsn
