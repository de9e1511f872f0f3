"""The anchor lists of the deformable backward (csrc/dcn_gather_kernels.h: a stable radix sort of the samples by anchor) through
lsn_dcn_anchor_lists, which routes and plans as lsn_dcn_backward does and runs the list construction alone.

What the lists must be follows from the keys the entry returns: with `anchor[s]` the anchor of sample s (-1: on no list),
    list_sample == the ids of the listed samples, stably sorted by anchor          (every list in ascending sample id)
    list_start  == searchsorted(sorted anchors, arange(anchors + 1))                (exclusive offsets; the last = listed samples)
-- integers, compared with torch.equal.  The keys themselves are checked against the sampling arithmetic in torch (fp32 products
and sums rounded one by one, as csrc/dcn_kernels.h tap_finish rounds them) wherever a case states its positions.

Shapes are the smallest that reach each structure of the sort: several 2048-sample blocks, a ragged last block and wave, one
list across eight blocks, no list at all, the -1 and last anchor rows, anchor counts on both sides of a digit boundary
(65 536 anchors: the sentinel key needs a 17th bit), sample ids with a deformable-group index."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle_py as orc  # noqa: E402
from lsnet_amd import _lib  # noqa: E402
from tests import backward_request_cases as br  # noqa: E402
from tests.test_ops_gpu import DCN_CASES, TOL, _dev, _err, _kernel_choice, _make  # noqa: E402

_CL = torch.channels_last
LSN_ERR_UNSUPPORTED = -2
BLOCK = 2048   # samples per workgroup of the sort (csrc/dcn_sort_plan.h DS_BLOCK)


def _case(name):
    return next(c for c in DCN_CASES if c['name'] == name)


class Launch:
    """One channels-last lsn_dcn_backward launch at the C ABI, built as HipBackend._dcn_backward_call builds it.  levels: dicts
    with x (B, C, H, W), off (B, dg 2 kh kw, Ho, Wo), optional mask, optional scale (sh, sw), want_gx (default True).  Levels whose
    x is the same tensor share one grad_input buffer.  k: the kernel (kh, kw)."""

    def __init__(self, levels, Co, groups=1, dg=1, stride=1, pad=1, dil=1, k=(3, 3)):
        from lsnet_amd.ops.hip_backend import HipBackend, _strides
        self.lib = _lib.load()
        dev = _dev()
        self.keep = []
        C = levels[0]['x'].shape[1]
        w = torch.zeros(Co, C // groups, k[0], k[1], device=dev).contiguous(memory_format=_CL)
        self.shape = HipBackend._shape(w, dict(stride=stride, pad=pad, dil=dil, groups=groups, dg=dg))
        self.n = len(levels)
        self.levels = (_lib.DcnLevel * self.n)()
        gxs = {}
        self.geom = []
        for L, lv in zip(self.levels, levels):
            x = lv['x'].to(dev).contiguous(memory_format=_CL)
            off = lv['off'].to(dev).contiguous(memory_format=_CL)
            mask = lv.get('mask')
            B, _, H, W = x.shape
            Ho, Wo = off.shape[2], off.shape[3]
            go = torch.zeros(B, Co, Ho, Wo, device=dev).contiguous(memory_format=_CL)
            L.input, L.offset, L.grad_output, L.off_st = x.data_ptr(), off.data_ptr(), go.data_ptr(), _strides(off)
            if mask is not None:
                mask = mask.to(dev).contiguous(memory_format=_CL)
                L.mask, L.mask_st = mask.data_ptr(), _strides(mask)
            if lv.get('want_gx', True):
                key = id(lv['x'])
                if key not in gxs:
                    gxs[key] = torch.empty_like(x)
                L.grad_input = gxs[key].data_ptr()
            L.B, L.H, L.W, L.Ho, L.Wo = B, H, W, Ho, Wo
            L.scale_h, L.scale_w = lv.get('scale', (1.0, 1.0))
            self.keep += [x, off, mask, go]
            self.geom.append((B, H, W, Ho, Wo))
        self.keep += [w, gxs]
        if _lib.split_math() and groups == 1:
            ws = torch.empty(2 * w.numel(), device=dev)
            self.shape.workspace = ws.data_ptr()
            self.keep.append(ws)
        self.ws_bytes = int(self.lib.lsn_dcn_backward_workspace_bytes(ctypes.byref(self.shape), self.n, self.levels))
        if self.ws_bytes > 0:
            gws = torch.empty(self.ws_bytes, device=dev, dtype=torch.uint8)
            self.shape.gather_workspace, self.shape.gather_workspace_bytes = gws.data_ptr(), self.ws_bytes
            self.keep.append(gws)

    def prepared_ok(self):
        return self.lib.lsn_dcn_prepared_ok(ctypes.byref(self.shape), self.n, self.levels, 1)

    def lists(self):
        """-> anchor[samples] (-1: no list), start[anchors + 1], the listed samples in list order, anchors"""
        from lsnet_amd.ops.hip_backend import _stream
        dev = _dev()
        counts = (ctypes.c_int64 * 2)()
        _lib.check(self.lib.lsn_dcn_anchor_lists(ctypes.byref(self.shape), self.n, self.levels, 1, None, None, None, counts, _stream()))
        ns, na = int(counts[0]), int(counts[1])
        anchor = torch.full((ns,), -7, dtype=torch.int32, device=dev)
        start = torch.full((na + 1,), -7, dtype=torch.int32, device=dev)
        sample = torch.full((ns,), -7, dtype=torch.int32, device=dev)
        _lib.check(self.lib.lsn_dcn_anchor_lists(ctypes.byref(self.shape), self.n, self.levels, 1, anchor.data_ptr(), start.data_ptr(),
                                                 sample.data_ptr(), counts, _stream()))
        torch.cuda.synchronize()
        assert (int(counts[0]), int(counts[1])) == (ns, na)
        return anchor.long(), start.long(), sample.long(), na


def check_lists(anchor, start, sample, na):
    """The three statements of the module docstring; returns the number of listed samples."""
    ns = anchor.numel()
    assert int(anchor.min()) >= -1 and int(anchor.max()) < na
    valid = anchor >= 0
    ids = torch.arange(ns, device=anchor.device)
    order = torch.sort(anchor[valid], stable=True)
    listed = int(valid.sum())
    assert torch.equal(sample[:listed], ids[valid][order.indices])
    assert bool((sample[listed:] == -1).all())
    want_start = torch.searchsorted(order.values.contiguous(), torch.arange(na + 1, device=anchor.device))
    assert torch.equal(start, want_start)
    assert int(start[na]) == listed
    return listed


def expected_anchor(launch, offs, dg=1, stride=1, pad=1, dil=1, k=(3, 3)):
    """Keys from the sampling arithmetic: sample (pixel, group, tap) of level l at py = fl(fl((ho s - p + i d) sh) + dy), tap
    (i, j) = divmod(tap, kw) of the kernel k = (kh, kw); its anchor is (floor(py) + 1, floor(px) + 1) on the (B, H + 1, W + 1) grid
    of its grad_input buffer.  One buffer per level here (the shared-buffer launches state their anchors themselves)."""
    out, abase = [], 0
    kh, kw = k
    K = kh * kw
    for (B, H, W, Ho, Wo), off, L in zip(launch.geom, offs, launch.levels):
        off = off.to(_dev()).float().view(B, dg, K, 2, Ho, Wo)
        k = torch.arange(K, device=off.device)
        ho = torch.arange(Ho, device=off.device).view(1, 1, 1, Ho, 1)
        wo = torch.arange(Wo, device=off.device).view(1, 1, 1, 1, Wo)
        by = (ho * stride - pad + (k // kw).view(1, 1, K, 1, 1) * dil).float() * torch.tensor(L.scale_h, dtype=torch.float32)
        bx = (wo * stride - pad + (k % kw).view(1, 1, K, 1, 1) * dil).float() * torch.tensor(L.scale_w, dtype=torch.float32)
        py, px = by + off[:, :, :, 0], bx + off[:, :, :, 1]
        inside = (py > -1) & (px > -1) & (py < H) & (px < W)
        b = torch.arange(B, device=off.device).view(B, 1, 1, 1, 1)
        a = abase + (b * (H + 1) + py.floor().long() + 1) * (W + 1) + px.floor().long() + 1
        a = torch.where(inside & bool(L.grad_input), a, torch.full_like(a, -1))
        out.append(a.permute(0, 3, 4, 1, 2).reshape(-1))   # (b, ho, wo, group, tap): ascending sample id
        abase += B * (H + 1) * (W + 1) if L.grad_input else 0     # (a level without grad_input has no anchor grid)
    return torch.cat(out)


def _route(launch, groups):
    """The list-building route of the launch.  The library's queries say whether there are lists (a gather workspace size
    above zero) and whether the matrix-pipe GEMM serves the call (lsn_dcn_prepared_ok: GATHER_MM); no query separates the
    other two, so `groups > 1 or exact-fp32 mode -> GATHER_GROUPED, else GATHER_XN` restates csrc/dcn_route.h route_backward here.
    A change of the routing rules fails the route assertions of this file for that reason, not because a list is wrong."""
    if launch.ws_bytes <= 0:
        return None
    if groups > 1 or not _lib.split_math():
        return 'GATHER_GROUPED'
    return 'GATHER_MM' if launch.prepared_ok() else 'GATHER_XN'


def _full_backward(levels, w, masks, go_seed=3, pyramid=False, dg=1, groups=1):
    """Every gradient of the launch through the op, twice: the two runs must agree bit for bit.  Returns the first run."""
    from lsnet_amd import ops
    dev = _dev()
    runs = []
    for _ in range(2):
        uniq = {}
        xs = []
        for lv in levels:
            if id(lv['x']) not in uniq:
                uniq[id(lv['x'])] = lv['x'].to(dev).contiguous(memory_format=_CL).requires_grad_()
            xs.append(uniq[id(lv['x'])])
        offs = [lv['off'].to(dev).contiguous(memory_format=_CL).requires_grad_() for lv in levels]
        msks = [None if m is None else m.to(dev).contiguous(memory_format=_CL).requires_grad_() for m in masks]
        wd = w.to(dev).contiguous(memory_format=_CL)
        outs = ops.dcn_multi(xs, offs, msks, wd, None, 1, 1, 1, groups, dg, scales=[lv.get('scale', (1.0, 1.0)) for lv in levels],
                             pyramid=pyramid)
        g = torch.Generator().manual_seed(go_seed)
        gos = [torch.randn(o.shape, generator=g).to(dev).contiguous(memory_format=_CL) for o in outs]
        wrt = list(uniq.values()) + offs + [m for m in msks if m is not None]
        grads = torch.autograd.grad(outs, wrt, gos)
        torch.cuda.synchronize()
        runs.append(([g_.clone() for g_ in grads], [g_.cpu() for g_ in gos], len(uniq)))
    for g0, g1 in zip(runs[0][0], runs[1][0]):
        assert torch.equal(g0, g1)
    return runs[0]


# ---------------------------------------------------------------------------------- (a) random offsets, one shape per route
ROUTE_CASES = [('GATHER_MM', 'default', _case('v2_head_p6')),
               ('GATHER_XN', 'x6_first_gemms', _case('v2_head_p6')),
               ('GATHER_GROUPED', 'default', _case('g4_c16')),
               ('GATHER_GROUPED', 'math_fp32', _case('v2_small'))]


@pytest.mark.parametrize('route,choice,case', ROUTE_CASES, ids=[f'{r}-{c}-{k["name"]}' for r, c, k in ROUTE_CASES])
def test_random_offsets_on_every_route(route, choice, case):
    with _kernel_choice(choice):
        x, w, b, off, mask, go, cfg = _make(case, _dev())
        launch = Launch([dict(x=x, off=off, mask=mask)], w.shape[0], groups=cfg['groups'], dg=cfg['dg'])
        assert _route(launch, cfg['groups']) == route
        anchor, start, sample, na = launch.lists()
        B, _, H, W = x.shape
        assert na == B * (H + 1) * (W + 1) and anchor.numel() == B * H * W * 9 * cfg['dg']
        listed = check_lists(anchor, start, sample, na)
        assert 0 < listed < anchor.numel()      # rand * 6 - 3 reaches outside the map
        assert anchor.numel() % BLOCK != 0      # (g) a ragged last block
        assert torch.equal(anchor, expected_anchor(launch, [off], dg=cfg['dg']))
        # the whole backward on these lists: bit-reproducible, and the oracle's gradients
        grads, gos, _ = _full_backward([dict(x=x, off=off)], w, [mask], groups=cfg['groups'], dg=cfg['dg'])
        ref = orc.deform_conv_backward(x, w, off, mask, gos[0], 1, 1, 1, cfg['groups'], cfg['dg'], 1.0, 1.0)
        names = ['gx', 'goff'] + (['gmask'] if mask is not None else [])
        errs = {n: _err(gt, ref[n]) for n, gt in zip(names, grads)}
        print(route, case['name'], errs)
        assert all(e < TOL for e in errs.values()), errs


# ---------------------------------------------------------------------------------- (b) converging samples
def _converge(B, Ho, Wo, scale, ty, tx):
    """Offsets that put every tap of every pixel at (ty, tx): dy = ty - (ho - 1 + i) scale, all on a quarter-pixel lattice (exact)."""
    k = torch.arange(9)
    by = (torch.arange(Ho).view(1, Ho, 1) - 1 + (k // 3).view(9, 1, 1)).float() * scale
    bx = (torch.arange(Wo).view(1, 1, Wo) - 1 + (k % 3).view(9, 1, 1)).float() * scale
    off = torch.stack([(ty - by).expand(9, Ho, Wo), (tx - bx).expand(9, Ho, Wo)], 1).reshape(1, 18, Ho, Wo)
    return off.repeat(B, 1, 1, 1).contiguous()


def test_converging_samples_one_list_over_eight_blocks():
    """Every tap of every pixel of a 40 x 40 map points into the interior of one source pixel: per image one list of 14 400
    entries, across eight 2048-sample blocks of the sort; all other lists are empty."""
    B, C, H, W = 2, 64, 40, 40
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, C, 3, 3, generator=g) * (1.0 / (3 * C ** 0.5))
    off = _converge(B, H, W, 1.0, 17.25, 23.5)
    with _kernel_choice('default'):
        launch = Launch([dict(x=x, off=off)], C)
        assert _route(launch, 1) == 'GATHER_MM'
        anchor, start, sample, na = launch.lists()
        assert check_lists(anchor, start, sample, na) == B * H * W * 9
        want = torch.arange(B, device=anchor.device).repeat_interleave(H * W * 9) * (H + 1) * (W + 1) + (17 + 1) * (W + 1) + 23 + 1
        assert torch.equal(anchor, want)
        assert int((start[1:] - start[:-1]).max()) == 14400 and 14400 > 7 * BLOCK
        grads, gos, _ = _full_backward([dict(x=x, off=off)], w, [None])
        ref = orc.deform_conv_backward(x, w, off, None, gos[0], 1, 1, 1, 1, 1, 1.0, 1.0)
        errs = {n: _err(gt, ref[n]) for n, gt in zip(['gx', 'goff'], grads)}
        print('converging', errs)
        assert all(e < TOL for e in errs.values()), errs


def test_converging_pyramid_levels_share_one_anchor_grid():
    """The same as a pyramid launch: destination levels of 40 x 40 and 20 x 20 pixels (scales 0.25 and 0.5) put every sample
    into one pixel of the 10 x 10 source map they share: per image ONE list with the samples of both levels, level 0 first."""
    B, C, H, W = 2, 64, 10, 10
    g = torch.Generator().manual_seed(12)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, C, 3, 3, generator=g) * (1.0 / (3 * C ** 0.5))
    levels = [dict(x=x, off=_converge(B, 40, 40, 0.25, 4.25, 6.5), scale=(0.25, 0.25)),
              dict(x=x, off=_converge(B, 20, 20, 0.5, 4.25, 6.5), scale=(0.5, 0.5))]
    with _kernel_choice('default'):
        launch = Launch(levels, C)
        assert _route(launch, 1) == 'GATHER_MM'
        anchor, start, sample, na = launch.lists()
        assert na == B * (H + 1) * (W + 1)      # one grid for both levels
        assert check_lists(anchor, start, sample, na) == B * (1600 + 400) * 9
        per = torch.arange(B, device=anchor.device) * (H + 1) * (W + 1) + (4 + 1) * (W + 1) + 6 + 1
        want = torch.cat([per.repeat_interleave(1600 * 9), per.repeat_interleave(400 * 9)])
        assert torch.equal(anchor, want)
        assert int((start[1:] - start[:-1]).max()) == (1600 + 400) * 9
        grads, gos, nx = _full_backward(levels, w, [None, None], pyramid=True)
        assert nx == 1
        refs = [orc.deform_conv_backward(x, w, lv['off'], None, go, 1, 1, 1, 1, 1, *lv['scale']) for lv, go in zip(levels, gos)]
        errs = {'gx': _err(grads[0], refs[0]['gx'] + refs[1]['gx']), 'goff0': _err(grads[1], refs[0]['goff']),
                'goff1': _err(grads[2], refs[1]['goff'])}
        print('converging pyramid', errs)
        assert all(e < TOL for e in errs.values()), errs


# ---------------------------------------------------------------------------------- (c) no sample on any list
def test_every_sample_outside_the_map():
    B, C, H, W = 2, 16, 13, 21
    x = torch.zeros(B, C, H, W)
    off = torch.full((B, 18, H, W), 1000.0)
    with _kernel_choice('default'):
        launch = Launch([dict(x=x, off=off)], 24)
        assert launch.ws_bytes > 0
        anchor, start, sample, na = launch.lists()
        assert check_lists(anchor, start, sample, na) == 0
        assert bool((anchor == -1).all()) and bool((start == 0).all()) and bool((sample == -1).all())


def test_level_without_grad_input_is_on_no_list():
    """Two levels, the second without grad_input: its samples get the sentinel key whatever their positions."""
    g = torch.Generator().manual_seed(13)
    B, C = 2, 16
    x0, x1 = torch.zeros(B, C, 13, 21), torch.zeros(B, C, 7, 9)
    off0, off1 = torch.rand(B, 18, 13, 21, generator=g) * 6 - 3, torch.rand(B, 18, 7, 9, generator=g) * 6 - 3
    with _kernel_choice('default'):
        launch = Launch([dict(x=x0, off=off0), dict(x=x1, off=off1, want_gx=False)], 24)
        assert launch.ws_bytes > 0
        anchor, start, sample, na = launch.lists()
        assert na == B * 14 * 22        # the second level has no anchor grid
        n0 = B * 13 * 21 * 9
        assert check_lists(anchor, start, sample, na) == int((anchor[:n0] >= 0).sum()) > 0
        assert bool((anchor[n0:] == -1).all())
        assert torch.equal(anchor, expected_anchor(launch, [off0, off1]))


# ---------------------------------------------------------------------------------- (d) border anchors
def test_border_anchor_rows_and_columns():
    """Positions in (-1, 0) and (H - 1, H): the anchors of row / column -1 and the last ones, corners included."""
    B, C, H, W = 2, 16, 9, 14
    g = torch.Generator().manual_seed(14)
    k = torch.arange(9)
    by = (torch.arange(H).view(1, H, 1) - 1 + (k // 3).view(9, 1, 1)).float().expand(9, H, W)
    bx = (torch.arange(W).view(1, 1, W) - 1 + (k % 3).view(9, 1, 1)).float().expand(9, H, W)
    pick = torch.randint(0, 3, (2, B, 9, H, W), generator=g)
    frac = torch.randint(1, 4, (2, B, 9, H, W), generator=g).float() * 0.25          # 0.25, 0.5, 0.75: exact
    inner = torch.stack([torch.randint(0, H - 1, (B, 9, H, W), generator=g), torch.randint(0, W - 1, (B, 9, H, W), generator=g)]).float()
    lo = torch.tensor([-1.0, -1.0]).view(2, 1, 1, 1, 1)
    hi = torch.tensor([H - 1.0, W - 1.0]).view(2, 1, 1, 1, 1)
    pos = torch.where(pick == 0, lo, torch.where(pick == 1, hi, inner)) + frac    # (-1, 0) / (H - 1, H) / inside
    off = torch.stack([pos[0] - by, pos[1] - bx], 2).reshape(B, 18, H, W)
    with _kernel_choice('default'):
        launch = Launch([dict(x=torch.zeros(B, C, H, W), off=off)], 24)
        assert launch.ws_bytes > 0
        anchor, start, sample, na = launch.lists()
        assert check_lists(anchor, start, sample, na) == anchor.numel()     # every position is inside (-1, H) x (-1, W)
        assert torch.equal(anchor, expected_anchor(launch, [off]))
        rem = anchor % ((H + 1) * (W + 1))
        rows, cols = rem // (W + 1), rem % (W + 1)
        for r, c in [(0, 0), (0, W), (H, 0), (H, W)]:       # the four corner anchors of the grid are hit
            assert bool(((rows == r) & (cols == c)).any()), (r, c)
        assert int(anchor.min()) == 0 and int(anchor.max()) == na - 1


# ---------------------------------------------------------------------------------- (e) digit boundaries
@pytest.mark.parametrize('B,HW,anchors', [(1, 255, 65536), (2, 181, 66248)])
def test_anchor_counts_around_two_to_the_sixteenth(B, HW, anchors):
    """65 536 anchors: the largest anchor id has 16 bits, the sentinel 17 -- digits of 9 + 9 bits, not 8 + 8."""
    g = torch.Generator().manual_seed(15)
    C = 64
    off = torch.rand(B, 18, HW, HW, generator=g) * 6 - 3
    with _kernel_choice('default'):
        launch = Launch([dict(x=torch.zeros(B, C, HW, HW), off=off)], C)
        assert launch.ws_bytes > 0
        anchor, start, sample, na = launch.lists()
        assert na == anchors
        listed = check_lists(anchor, start, sample, na)
        assert 0 < listed < anchor.numel()
        assert torch.equal(anchor, expected_anchor(launch, [off]))
        assert int(anchor.max()) >= 1 << 16 or na == 1 << 16      # keys above the 16-bit range where there are such anchors


# ---------------------------------------------------------------------------------- (f) deformable groups
def test_sample_ids_with_a_group_index():
    case = _case('v2_dg2_co256')
    with _kernel_choice('default'):
        x, w, b, off, mask, go, cfg = _make(case, _dev())
        assert cfg['dg'] == 2
        launch = Launch([dict(x=x, off=off, mask=mask)], w.shape[0], dg=2)
        assert launch.ws_bytes > 0
        anchor, start, sample, na = launch.lists()
        assert anchor.numel() == x.shape[0] * x.shape[2] * x.shape[3] * 18
        assert 0 < check_lists(anchor, start, sample, na) < anchor.numel()
        assert torch.equal(anchor, expected_anchor(launch, [off], dg=2))


# ---------------------------------------------------------------------------------- (g) tiny launches
def test_launch_smaller_than_one_block():
    """A 3 x 3 map, one image: 81 samples -- one block, a second wave of 17 lanes."""
    g = torch.Generator().manual_seed(16)
    off = torch.rand(1, 18, 3, 3, generator=g) * 6 - 3
    with _kernel_choice('default'):
        launch = Launch([dict(x=torch.zeros(1, 16, 3, 3), off=off)], 24)
        assert launch.ws_bytes > 0
        anchor, start, sample, na = launch.lists()
        assert anchor.numel() == 81 and na == 16
        assert 0 < check_lists(anchor, start, sample, na) < 81
        assert torch.equal(anchor, expected_anchor(launch, [off]))


def test_routes_without_lists_are_refused():
    """The scatter routes build no lists: no gather workspace, or offset gradients without grad_input."""
    from lsnet_amd.ops.hip_backend import _stream
    g = torch.Generator().manual_seed(17)
    off = torch.rand(2, 18, 7, 9, generator=g) * 6 - 3
    with _kernel_choice('default'):
        launch = Launch([dict(x=torch.zeros(2, 16, 7, 9), off=off)], 24)
        assert launch.ws_bytes > 0
        launch.shape.gather_workspace, launch.shape.gather_workspace_bytes = None, 0
        counts = (ctypes.c_int64 * 2)()
        rc = launch.lib.lsn_dcn_anchor_lists(ctypes.byref(launch.shape), 1, launch.levels, 1, None, None, None, counts, _stream())
        assert rc == LSN_ERR_UNSUPPORTED and b'lsn_dcn_anchor_lists' in launch.lib.lsn_last_error()
        launch = Launch([dict(x=torch.zeros(2, 16, 7, 9), off=off)], 24)      # lists there are, but not in the reference layout
        rc = launch.lib.lsn_dcn_anchor_lists(ctypes.byref(launch.shape), 1, launch.levels, 0, None, None, None, counts, _stream())
        assert rc == LSN_ERR_UNSUPPORTED and b'LSN_NHWC' in launch.lib.lsn_last_error()
    with _kernel_choice('x3_atomic_fallbacks'):
        launch = Launch([dict(x=torch.zeros(2, 16, 7, 9), off=off)], 24)
        assert launch.ws_bytes == 0
        rc = launch.lib.lsn_dcn_anchor_lists(ctypes.byref(launch.shape), 1, launch.levels, 1, None, None, None, counts, _stream())
        assert rc == LSN_ERR_UNSUPPORTED


def test_request_case_shapes_build_their_lists():
    """The cases of tests/backward_request_cases.py ('mm', 'mm_wg', 'grouped', 'xn', 'v1'; 7 x 9 and 6 x 10 maps): under the
    defaults they cover all three list-building routes between them."""
    with _kernel_choice('default'):
        routes = set()
        for name, case in br.DCN.items():
            c = br.cfg_of(case)
            built = br.build(case)
            x, off, mask = built.leaves['x'], built.leaves['off'], built.leaves.get('mask')
            launch = Launch([dict(x=x, off=off, mask=mask)], c['Co'], groups=c['groups'])
            routes.add(_route(launch, c['groups']))
            anchor, start, sample, na = launch.lists()
            assert 0 < check_lists(anchor, start, sample, na) < anchor.numel(), name
            assert torch.equal(anchor, expected_anchor(launch, [off])), name
        assert routes == {'GATHER_MM', 'GATHER_XN', 'GATHER_GROUPED'}, routes
