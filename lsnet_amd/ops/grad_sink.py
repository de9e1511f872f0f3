"""Parameter-gradient sinks: let the kernel that produces a parameter's gradient ADD it straight into the buffer the
optimizer (and the all-reduce) will read, instead of handing a fresh tensor to autograd.

With `BucketedGradReducer` every `p.grad` is a view into a flat bucket that is zeroed once per step.  Returning a new
`grad_weight` from a custom autograd Function then costs, per parameter and step, an allocation, a memset (the weight-
gradient kernels accumulate over pixel ranges), and autograd's `p.grad.add_(grad_weight)`.  The operators of this package
make a `claim` per backward call instead: when every wanted parameter's `.grad` IS its registered sink they call the
`accumulate = 1` form of the C entry point on the sinks (include/lsnet_hip.h: lsn_conv2d_backward_weight ...) and return
None for those inputs; `done(p)` tells the owner of the sink (the reducer counts a parameter's uses per step to launch
bucket all-reduces early).  `claim` is the only caller of `sink` and `done` in the package.
Anything else -- no reducer, `p.grad` replaced by the user, an operator without sink support -- keeps the classic path,
and the two mix freely because both ADD into the same buffer."""


def register(p, view, on_done=None):
    """`view` is where p's gradient lives for the coming backward passes (the caller zeroes it per step)."""
    p._lsn_sink = view
    p._lsn_sink_done = on_done


def unregister(p):
    for k in ('_lsn_sink', '_lsn_sink_done'):
        if hasattr(p, k):
            delattr(p, k)


def sink(p):
    """The tensor to accumulate p's gradient into, or None."""
    s = getattr(p, '_lsn_sink', None)
    if s is None or p.grad is not s:
        return None
    return s


def done(p):
    cb = getattr(p, '_lsn_sink_done', None)
    if cb is not None:
        cb(p)


class claim:
    """Where ONE backward call's parameter gradients go, decided once.  params: [(parameter or None, is its gradient
    wanted)]; optional: positions that may be unwanted (a bias); allowed: whatever else the site needs for sinks at all.
    accumulate = 1: `sinks` holds every wanted parameter's registered sink (None where unwanted) and the kernel ADDS
    into them; it takes all of these: every other parameter wanted, a live sink for every wanted one, each sink with
    its parameter's strides.  Otherwise accumulate = 0, `sinks` is all None and the site writes buffers of its own."""
    __slots__ = ('params', 'sinks', 'accumulate')

    def __init__(self, params, optional=(), allowed=True):
        self.params = params
        ok, sinks = bool(allowed), []
        for i, (p, want) in enumerate(params):      # (a plain loop: this runs in every backward node of a step)
            s = None
            if want and p is not None:
                s = sink(p)
                ok = ok and s is not None and s.stride() == p.stride()
            else:
                ok = ok and i in optional
            sinks.append(s)
        self.accumulate = 1 if ok else 0
        self.sinks = sinks if ok else [None] * len(sinks)

    def results(self, fresh=()):
        """What goes back to autograd, one entry per parameter, after the kernel ran.  Accumulated: None for all, and each
        sink's owner is told `done` once.  Else `fresh` (the site's buffers, in order) where wanted, None elsewhere."""
        if self.accumulate:
            for (p, _), s in zip(self.params, self.sinks):
                if s is not None:
                    done(p)
            return (None,) * len(self.sinks)
        return tuple(g if want else None for (_, want), g in zip(self.params, fresh))
