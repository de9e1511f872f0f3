"""Case tables and the fp64 reference of the dense-convolution geometry tests (tests/test_conv_geometry_host.py,
tests/test_conv_geometry_gpu.py).

tests/test_ops_gpu.py CONV_CASES walks one line through the family that ops/conv.py hip_conv_ok admits: square kernels with
their natural padding, B <= 2.  The tables here leave that line: rectangular taps, padding beyond and short of natural,
even kernels and strides beyond the kernel, dilation, one-pixel maps, batches whose images share a pixel tile, the channel
counts around the kernels' 4- and 8-channel granularities, and the row-merged form of the shallow convolutions.

Sizes: the smallest at which a launch still has two pixel tiles with a ragged last one -- input AND output at least
9 x 11 at B = 3 (297 pixels: three 128-pixel tiles, five 64-pixel ones) -- so that the whole table costs seconds.  Every
geometry of groups 1 .. 6 meets the four forward tiles of csrc/conv_route.h conv_route (Co <= 32, <= 64, wider, Co % 256 == 0)
through Co = 24, 48, 136, 256, with C alternating between 32 (one 32-channel chunk) and 72 (a partial third chunk); one row
per group has C = 64, Co = 256 and >= 4096 output pixels, which is where csrc/conv_wgrad_route.h cw_dense_mm_ok takes the
weight gradient of a kernel with nine taps or more (group 7 is about narrow channel counts and has no such row).

The reference is F.conv2d in fp64 on the CPU -- never the code under test."""
import collections

import torch
import torch.nn.functional as F

Case = collections.namedtuple('Case', 'group B C Co kh kw s p d H W bias seed')

TILE_CO = (24, 48, 136, 256)
TILE_C = (32, 72)


def case_id(c):
    return f'g{c.group}-B{c.B}-C{c.C}-Co{c.Co}-k{c.kh}x{c.kw}-s{c.s}-p{c.p}-d{c.d}-{c.H}x{c.W}' + ('-b' if c.bias else '')


def out_size(n, k, s, p, d):
    return (n + 2 * p - (d * (k - 1) + 1)) // s + 1


def out_shape(c):
    return c.B, c.Co, out_size(c.H, c.kh, c.s, c.p, c.d), out_size(c.W, c.kw, c.s, c.p, c.d)


def _fit(out, k, s, p, d, extra):
    """the input size that gives `out` outputs and leaves `extra` (< s) trailing pixels no window reaches"""
    return (out - 1) * s + d * (k - 1) + 1 - 2 * p + extra


def _tiled(group, geoms, B=3):
    """every geometry (kh, kw, s, p, d) at the four forward tiles; input and output at least 9 x 11"""
    cases = []
    for gi, (kh, kw, s, p, d) in enumerate(geoms):
        H = max(9, _fit(9, kh, s, p, d, gi % s))
        W = max(11, _fit(11, kw, s, p, d, (gi + 1) % s))
        for ti, Co in enumerate(TILE_CO):
            n = gi * len(TILE_CO) + ti
            cases.append(Case(group, B, TILE_C[(gi + ti) % 2], Co, kh, kw, s, p, d, H, W, n % 3 != 0, 1000 * group + n))
    return cases


def _wide(group, B, kh, kw, s, p, d, H, W):
    """C = 64 -> Co = 256 at >= 4096 output pixels: the weight gradient on the fragment-order kernel"""
    c = Case(group, B, 64, 256, kh, kw, s, p, d, H, W, True, 1000 * group + 999)
    assert c.B * out_shape(c)[2] * out_shape(c)[3] >= 4096 and kh * kw >= 9
    return c


# 1: rectangular taps -- i * kw + j tap masks, per-axis residue classes (ni != nj), the general weight-gradient kernel
RECT = _tiled(1, [(kh, kw, s, p, 1) for kh, kw in ((1, 3), (3, 1), (1, 7), (7, 1), (3, 5), (5, 3), (2, 3)) for s in (1, 2)
                  for p in (0, 1)]) + [_wide(1, 1, 3, 5, 1, 1, 1, 66, 67)]

# 2: padding other than natural -- none under a 3x3 and a 5x5, beyond (k - 1) dil (a negative pad for the data gradient's
# forward kernel), any under a 1x1
PAD = _tiled(2, [(k, k, s, p, 1) for k, p in ((3, 0), (3, 2), (3, 3), (1, 1), (1, 2), (5, 0)) for s in (1, 2)]) \
    + [_wide(2, 1, 3, 3, 1, 0, 1, 66, 67)]

# 3: even kernels and strides beyond the kernel -- one tap per residue class, classes without a tap beside them
EVEN = _tiled(3, [(2, 2, 2, 0, 1), (2, 2, 1, 1, 1), (4, 4, 2, 1, 1), (4, 4, 4, 0, 1), (1, 1, 3, 0, 1), (3, 3, 4, 1, 1),
                  (2, 2, 3, 0, 1), (3, 3, 3, 2, 2)]) \
    + [Case(3, 3, 8, 24, 8, 8, 8, 0, 1, _fit(9, 8, 8, 0, 1, 5), _fit(11, 8, 8, 0, 1, 0), True, 3998),   # 64 taps, 64 classes
       _wide(3, 1, 4, 4, 2, 1, 1, 130, 130)]

# 4: dilation
DIL = _tiled(4, [(3, 3, 1, 3, 3), (3, 3, 1, 0, 2), (5, 5, 2, 4, 2)]) + [_wide(4, 1, 3, 3, 1, 3, 3, 66, 66)]


def _maps(group, rows, B=3):
    cases = []
    for gi, (kh, kw, p, H, W) in enumerate(rows):
        for ti, Co in enumerate(TILE_CO):
            n = gi * len(TILE_CO) + ti
            cases.append(Case(group, B, TILE_C[(gi + ti) % 2], Co, kh, kw, 1, p, 1, H, W, n % 3 != 0, 1000 * group + n))
    return cases


# 5: degenerate maps -- a single row, a single column, a single pixel (one live tap of nine), a single output pixel, a map
# smaller than the kernel
DEGEN = _maps(5, [(3, 3, 1, 1, 37), (3, 3, 1, 37, 1), (3, 3, 1, 1, 1), (1, 1, 0, 1, 1), (5, 5, 0, 5, 5), (5, 5, 2, 2, 3)]) \
    + [_wide(5, 1, 3, 3, 1, 1, 1, 1, 4100)]

# 6: batches of few pixels per image -- a pixel tile spans several images
BATCH = [c for B in (3, 5, 8) for c in _maps(6, [(3, 3, 1, 5, 7), (1, 1, 0, 5, 7)], B)]
BATCH = [c._replace(seed=6000 + i) for i, c in enumerate(BATCH)] + [_wide(6, 5, 3, 3, 1, 1, 1, 29, 29)]

# 7: channel edges -- the zero-filter padding of the data gradient (Co % 4 != 0 with C <= 64; C = 68 is beyond it), channel
# counts below one 32-channel chunk, C % 4 != 0 with gradients
CHAN = [Case(7, 3, C, Co, k, k, 1, k // 2, 1, 9, 11, (C + Co) % 2 == 0, 7000 + 100 * i + 10 * j + k)
        for i, Co in enumerate((1, 2, 3, 5, 6)) for j, C in enumerate((4, 8, 12, 64, 68)) for k in (3, 1)] \
    + [Case(7, 3, C, Co, k, k, 1, k // 2, 1, 9, 11, True, 7500 + 100 * i + 10 * j + k)
       for i, C in enumerate((1, 2, 5, 6, 7)) for j, Co in enumerate((16, 96)) for k in (3, 1)]

GENERIC = RECT + PAD + EVEN + DIL + DEGEN + BATCH + CHAN

# 8: the row-merged form (ops/conv.py _stem_forward: C < 8, kw > 1, dilation 1, no gradient): C, kh, kw, s, p, Co, relu, bias
_ROWS = [(3, 7, 7, 2, 3, 64, False, False), (3, 7, 7, 1, 3, 27, True, True), (1, 3, 3, 1, 1, 8, False, True),
         (1, 5, 5, 2, 0, 96, True, False), (4, 3, 3, 2, 1, 64, True, True), (4, 3, 5, 1, 1, 27, False, False),
         (5, 3, 3, 3, 0, 96, False, True), (5, 5, 5, 1, 4, 8, True, False), (7, 3, 3, 1, 4, 27, True, True),
         (7, 7, 7, 3, 3, 64, False, False), (3, 1, 3, 1, 1, 96, False, True), (3, 1, 3, 2, 0, 8, True, False),
         (1, 1, 3, 3, 1, 64, False, False), (7, 3, 5, 2, 3, 96, True, True), (4, 5, 5, 3, 1, 27, False, True),
         (5, 1, 3, 1, 0, 64, True, True), (3, 3, 5, 3, 4, 8, False, False), (1, 7, 7, 1, 0, 27, True, False),
         (4, 7, 7, 2, 4, 96, False, True), (7, 5, 5, 2, 1, 8, True, True), (3, 3, 3, 1, 0, 64, False, True)]
ROW_MERGED = [(Case(8, 2, C, Co, kh, kw, s, p, 1, max(9, _fit(9, kh, s, p, 1, i % s)), max(11, _fit(11, kw, s, p, 1, (i + 1) % s)),
                    bias, 8000 + i), relu) for i, (C, kh, kw, s, p, Co, relu, bias) in enumerate(_ROWS)]

ALL = GENERIC + [c for c, _ in ROW_MERGED]


def inputs(c):
    """(x, w, b or None, go): fp32 CPU tensors from the case's own seed; weights scaled for outputs of order one"""
    g = torch.Generator().manual_seed(c.seed)
    x = torch.randn(c.B, c.C, c.H, c.W, generator=g)
    w = torch.randn(c.Co, c.C, c.kh, c.kw, generator=g) / (c.C * c.kh * c.kw) ** 0.5
    b = torch.randn(c.Co, generator=g) if c.bias else None
    go = torch.randn(out_shape(c), generator=g)
    return x, w, b, go


GATE_MARGIN = 1e-3


def gate_safe(pre, go):
    """go with zeros wherever the fp64 pre-activation lies within GATE_MARGIN of the output range of zero: a ReLU gate that
    fp32 arithmetic could put on the other side carries no gradient, so every element can be held by the maximum."""
    return go * (pre.abs() > GATE_MARGIN * pre.abs().max()).to(go.dtype)


def ref(x, w, b, s, p, d, go, relu):
    """F.conv2d (+ ReLU) in fp64 on the CPU -> (y, gx, gw, gb or None).  relu: `go` goes through gate_safe first."""
    x = x.detach().double().cpu().requires_grad_()
    w = w.detach().double().cpu().contiguous().requires_grad_()
    b = None if b is None else b.detach().double().cpu().requires_grad_()
    go = go.detach().double().cpu()
    y = F.conv2d(x, w, b, s, p, d)
    if relu:
        go = gate_safe(y.detach(), go)
        y = F.relu(y)
    g = torch.autograd.grad(y, [x, w] + ([b] if b is not None else []), go)
    return y.detach(), g[0], g[1], (g[2] if b is not None else None)


_refs = {}


def reference(c, relu=False):
    """The shared reference of a case: (x, w, b, go as the backward pass gets it, (y, gx, gw, gb)).  Computed once."""
    key = (c, relu)
    if key not in _refs:
        x, w, b, go = inputs(c)
        if relu:
            with torch.no_grad():
                go = gate_safe(F.conv2d(x.double(), w.double(), None if b is None else b.double(), c.s, c.p, c.d), go.double()).float()
        _refs[key] = (x, w, b, go, ref(x, w, b, c.s, c.p, c.d, go, relu))
    return _refs[key]


# ---- plausible mistakes, as fp64 functions of (x, w, b): what tests/test_conv_geometry_host.py holds every case against ----
def _windows(x, w, b, c, top, left):
    """The convolution as a kernel computes it -- window (ho, wo) starts at input row ho s - top, column wo s - left, zeros
    outside the map -- on the case's own output grid.  top = left = p is the convolution itself."""
    _, _, Ho, Wo = out_shape(c)
    eh, ew = c.d * (w.shape[2] - 1) + 1, c.d * (w.shape[3] - 1) + 1
    bottom = max(0, (Ho - 1) * c.s - top + eh - c.H)
    right = max(0, (Wo - 1) * c.s - left + ew - c.W)
    y = F.conv2d(F.pad(x, (left, right, top, bottom)), w, b, c.s, 0, c.d)     # (negative pads crop)
    return y[:, :, :Ho, :Wo]


def mistaken(kind, x, w, b, c):
    if kind == 'taps_transposed':        # tap (i, j) applied at offset (j, i)
        K = max(c.kh, c.kw)
        wt = F.pad(w, (0, K - c.kw, 0, K - c.kh)).transpose(2, 3)
        return _windows(x, wt, b, c, c.p, c.p)
    if kind == 'pad_plus_one':           # windows start one pixel early
        return _windows(x, w, b, c, c.p + 1, c.p + 1)
    if kind == 'phase_shifted':          # windows start one pixel late
        return _windows(x, w, b, c, c.p - 1, c.p - 1)
    if kind == 'images_swapped':
        return F.conv2d(x.roll(1, 0), w, b, c.s, c.p, c.d)
    if kind == 'last_channel_dropped':
        y = F.conv2d(x, w, b, c.s, c.p, c.d)
        return torch.cat([y[:, :-1], torch.zeros_like(y[:, -1:])], 1)
    if kind == 'last_channel_duplicated':
        y = F.conv2d(x, w, b, c.s, c.p, c.d)
        return torch.cat([y[:, :-1], y[:, -2:-1]], 1)
    raise KeyError(kind)


MISTAKES = {1: ('taps_transposed',), 8: ('taps_transposed',), 2: ('pad_plus_one',), 5: ('pad_plus_one',), 3: ('phase_shifted',),
            4: ('phase_shifted',), 6: ('images_swapped',), 7: ('last_channel_dropped', 'last_channel_duplicated')}


def mistaken_ref(kind, c):
    """(y, gx, gw) of the mistaken operator in fp64, under the case's inputs and output gradient"""
    x, w, b, go = inputs(c)
    x, w = x.double().requires_grad_(), w.double().requires_grad_()
    y = mistaken(kind, x, w, None if b is None else b.double(), c)
    gx, gw = torch.autograd.grad(y, [x, w], go.double(), allow_unused=True)
    return y.detach(), (torch.zeros_like(x) if gx is None else gx), (torch.zeros_like(w) if gw is None else gw)


def rel_diff(a, b):
    """max |a - b| over the range of b: tests/test_ops_gpu.py _err"""
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-12)
