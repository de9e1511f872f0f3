"""The deformable kernels at kernel sizes other than 3 x 3 (tests/dcn_kernel_size_cases.py) against the CPU oracle, which
tests/test_dcn_kernel_sizes_host.py pins at these sizes: 1x1, 2x2, 1x3, 3x1, 4x4, 5x5, 7x7 and 8x8 kernels, KD = kh kw dg from 1 to 64
(and 75: refused), under the five kernel choices of tests/test_ops_gpu.py.

 * parity through the op (both layouts): output and all five gradients at that file's TOL;
 * the C ABI serves a call or refuses it as a whole: a refused call (LSN_ERR_UNSUPPORTED) has written to none of its outputs,
   gradients or workspaces, its message names the LDS need or the bound, and it stands in EXPECTED_REFUSALS -- every row of
   which is in fact refused; no call at or below LSN_DCN_KD_EVERY_ROUTE is ever refused;
 * the route the queries let one observe is the one the cases file derives from csrc/dcn_route.h;
 * the anchor lists at KD = 1, 25 and 50 against the restatement of tests/test_dcn_lists_gpu.py;
 * the eight reference-named entry points with a 1x3 and a 3x1 kernel: a kW / kH swap changes the output shape or the values."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle_py as orc  # noqa: E402
from lsnet_amd import _lib  # noqa: E402
from tests import dcn_kernel_size_cases as ks  # noqa: E402
from tests.test_dcn_lists_gpu import Launch, check_lists, expected_anchor  # noqa: E402
from tests.test_ops_gpu import KERNEL_CHOICES, TOL, _dev, _kernel_choice, _report, _to  # noqa: E402
from tests.test_ops_gpu import dcn_kernel_choice  # noqa: E402,F401  (the fixture: every choice, restored afterwards)

LSN_ERR_UNSUPPORTED = -2
SENTINEL = -7.25        # what every output buffer holds before a call
SENTINEL_BYTE = 0xA5    # ... and every byte of a workspace


def _grad_names(mask, b):
    return ['gx', 'goff'] + (['gmask'] if mask is not None else []) + ['gw'] + (['gb'] if b is not None else [])


# ------------------------------------------------------------------------------------------------------ parity through the op
@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('name', ks.NAMES)
def test_parity(name, layout, dcn_kernel_choice):
    """ops.dcn_multi + torch.autograd.grad against the oracle.  A pass that EXPECTED_REFUSALS lists raises instead, with the
    library's message; everything in front of it is still compared."""
    from lsnet_amd import ops
    dev = _dev()
    cl = layout == 'nhwc'
    (x, w, b, off, mask, go, cfg), ref, gref = ks.reference(name)
    xd, wd, od, md = _to(x, dev, cl).requires_grad_(), _to(w, dev, cl).requires_grad_(), _to(off, dev, cl).requires_grad_(), \
        _to(mask, dev, cl)
    bd = None if b is None else b.to(dev).requires_grad_()
    if md is not None:
        md.requires_grad_()

    def forward():
        return ops.dcn_multi([xd], [od], [md], wd, bd, cfg['stride'], cfg['pad'], cfg['dil'], cfg['groups'], cfg['dg'],
                             scales=[(cfg['sh'], cfg['sw'])], pyramid=cfg['pyramid'])[0]

    refused_fwd = ks.EXPECTED_REFUSALS.get((name, dcn_kernel_choice, 'fwd'))
    if refused_fwd:
        with pytest.raises(RuntimeError, match=refused_fwd):
            forward()
        return
    out = forward()
    torch.cuda.synchronize()
    errs = {'out': _report(name + '/out', out, ref)}
    wrt = [t for t in (xd, od, md, wd, bd) if t is not None]
    refused_bwd = ks.EXPECTED_REFUSALS.get((name, dcn_kernel_choice, 'bwd'))
    if refused_bwd:
        with pytest.raises(RuntimeError, match=refused_bwd):
            torch.autograd.grad(out, wrt, _to(go, dev, cl))
    else:
        grads = torch.autograd.grad(out, wrt, _to(go, dev, cl))
        torch.cuda.synchronize()
        for n, gt in zip(_grad_names(mask, b), grads):
            errs[n] = _report(name + '/' + n, gt, gref[n])
    print('PARITY', name, layout, dcn_kernel_choice, 'bwd refused' if refused_bwd else 'served',
          {k: f'{v:.1e}' for k, v in errs.items()})
    assert all(e < TOL for e in errs.values()), errs


# ------------------------------------------------------------------------------------------------------ the C ABI, one level
class _Call:
    """One channels-last level of a case at the C ABI, built as HipBackend builds it (shape from the weight, workspace sizes
    from the library's own answers); every output, gradient and workspace pre-filled with a sentinel."""

    def __init__(self, name):
        from lsnet_amd.ops.hip_backend import HipBackend, _ptr, _strides
        self.lib = _lib.load()
        dev = _dev()
        (x, w, b, off, mask, go, cfg), self.ref, self.gref = ks.reference(name)
        self.name, self.cfg, self.has_mask, self.has_bias = name, cfg, mask is not None, b is not None
        self.xd, self.wd, self.od, self.md, self.gd = (_to(t, dev, True) for t in (x, w, off, mask, go))
        self.bd = None if b is None else b.to(dev)
        self._ptr, self._strides, self._shape = _ptr, _strides, HipBackend._shape
        self.B, self.Co, (self.Ho, self.Wo) = x.shape[0], w.shape[0], cfg['out_hw']
        self.split = _lib.split_math()

    def fresh(self):
        shape = self._shape(self.wd, self.cfg)
        levels = (_lib.DcnLevel * 1)()
        L = levels[0]
        L.input, L.offset, L.mask, L.off_st = self._ptr(self.xd), self._ptr(self.od), self._ptr(self.md), self._strides(self.od)
        if self.md is not None:
            L.mask_st = self._strides(self.md)
        L.B, L.H, L.W, L.Ho, L.Wo = self.B, self.xd.shape[2], self.xd.shape[3], self.Ho, self.Wo
        L.scale_h, L.scale_w = self.cfg['sh'], self.cfg['sw']
        return shape, levels, L

    def _workspace(self, nbytes):
        return torch.full((nbytes,), SENTINEL_BYTE, dtype=torch.uint8, device=self.xd.device) if nbytes > 0 else None

    def forward(self):
        """-> rc, message, out, the buffers a refused call must have left alone, lsn_dcn_prepared_ok(forward)"""
        from lsnet_amd.ops.hip_backend import _stream
        shape, levels, L = self.fresh()
        ws = self._workspace(8 * self.wd.numel() if self.split else 0)
        out = torch.full((self.B, self.Co, self.Ho, self.Wo), SENTINEL, device=self.xd.device).contiguous(memory_format=torch.channels_last)
        shape.workspace, L.output = self._ptr(ws), self._ptr(out)
        prepared = self.lib.lsn_dcn_prepared_ok(ctypes.byref(shape), 1, levels, 0)
        rc = self.lib.lsn_dcn_forward(ctypes.byref(shape), 1, levels, self._ptr(self.wd), self._ptr(self.bd), 1, _stream())
        msg = self.lib.lsn_last_error().decode('utf-8', 'replace') if rc else ''
        torch.cuda.synchronize()
        return rc, msg, out, {'out': out, 'workspace': ws}, prepared

    def backward(self):
        """-> rc, message, {name: gradient}, the buffers a refused call must have left alone, the three query answers"""
        from lsnet_amd.ops.hip_backend import _stream
        full = lambda t: None if t is None else torch.full_like(t, SENTINEL)   # noqa: E731  (keeps channels-last)
        g = dict(gx=full(self.xd), goff=full(self.od), gmask=full(self.md), gw=full(self.wd),
                 gb=None if self.bd is None else torch.full((self.Co,), SENTINEL, device=self.xd.device))
        shape, levels, L = self.fresh()
        L.grad_output, L.grad_input, L.grad_offset, L.grad_mask = (self._ptr(t) for t in (self.gd, g['gx'], g['goff'], g['gmask']))
        ws = self._workspace(8 * self.wd.numel() if (self.split and self.cfg['groups'] == 1) else 0)
        shape.workspace = self._ptr(ws)
        nbytes = int(self.lib.lsn_dcn_backward_workspace_bytes(ctypes.byref(shape), 1, levels))
        gws = self._workspace(nbytes)
        if gws is not None:
            shape.gather_workspace, shape.gather_workspace_bytes = gws.data_ptr(), nbytes
        queries = dict(ws_bytes=nbytes, prepared=self.lib.lsn_dcn_prepared_ok(ctypes.byref(shape), 1, levels, 1),
                       pitched=self.lib.lsn_dcn_pitched_ok(ctypes.byref(shape), 1, levels, 1))
        rc = self.lib.lsn_dcn_backward(ctypes.byref(shape), 1, levels, self._ptr(self.wd), self._ptr(g['gw']), self._ptr(g['gb']), 1,
                                       _stream())
        msg = self.lib.lsn_last_error().decode('utf-8', 'replace') if rc else ''
        torch.cuda.synchronize()
        grads = {k: v for k, v in g.items() if v is not None}
        return rc, msg, grads, dict(grads, workspace=ws, gather_workspace=gws), queries


def _untouched(buffers):
    for k, t in buffers.items():
        if t is not None:
            want = SENTINEL_BYTE if t.dtype == torch.uint8 else SENTINEL
            assert bool((t == want).all()), f'{k}: a refused call wrote to it'


@pytest.mark.parametrize('choice', list(KERNEL_CHOICES))
@pytest.mark.parametrize('name', ks.NAMES)
def test_served_or_refused_cleanly(name, choice):
    """lsn_dcn_forward and lsn_dcn_backward on sentinel-filled buffers: served (and right), or refused with every buffer intact,
    a message that names the cause, and a row in EXPECTED_REFUSALS; the table holds no row that is served.  Where the call is
    served, what the queries say of its route is what the cases file derives from csrc/dcn_route.h."""
    with _kernel_choice(choice):
        call = _Call(name)
        served = {}
        # ---- forward
        rc, msg, out, buffers, prepared_fwd = call.forward()
        want = ks.EXPECTED_REFUSALS.get((name, choice, 'fwd'))
        print('ABI', name, choice, 'fwd', 'refused: ' + msg if rc else 'served')
        assert rc in (0, LSN_ERR_UNSUPPORTED), (rc, msg)
        assert (rc != 0) == (want is not None), f'forward: returned {rc} {msg!r}, EXPECTED_REFUSALS says {want!r}'
        if rc:
            _untouched(buffers)
            assert want in msg, msg
        else:
            assert _report(name + '/abi_out', out, call.ref) < TOL
        served['fwd'] = rc == 0
        # ---- backward
        rc, msg, grads, buffers, queries = call.backward()
        want = ks.EXPECTED_REFUSALS.get((name, choice, 'bwd'))
        print('ABI', name, choice, 'bwd', 'refused: ' + msg if rc else 'served', queries)
        assert rc in (0, LSN_ERR_UNSUPPORTED), (rc, msg)
        assert (rc != 0) == (want is not None), f'backward: returned {rc} {msg!r}, EXPECTED_REFUSALS says {want!r}'
        if rc:
            _untouched(buffers)
            assert want in msg, msg
        else:
            errs = {n: _report(name + '/abi_' + n, grads[n], call.gref[n]) for n in _grad_names(call.md, call.bd)}
            assert all(e < TOL for e in errs.values()), errs
        served['bwd'] = rc == 0
        # ---- the bound of include/lsnet_hip.h: at or below it nothing is refused, under any choice
        if ks.kd(ks.case(name)) <= ks.kd_every_route():
            assert served == {'fwd': True, 'bwd': True}, served
        # ---- the observable part of the route
        if name in ks.ROUTES:
            fwd, data, wgrad = ks.ROUTES[name][choice]
            assert prepared_fwd == (1 if fwd == 'FWD_MM' else 0), (fwd, prepared_fwd)
            assert queries['prepared'] == (1 if data == 'GATHER_MM' else 0), (data, queries)
            assert (queries['ws_bytes'] > 0) == data.startswith('GATHER_'), (data, queries)
            # (out_pitch in a call that asks for grad_weight: the column gradients AND the weight gradient on the matrix pipe)
            assert queries['pitched'] == (1 if (data == 'GATHER_MM' and wgrad == 'WG_MM') else 0), (data, wgrad, queries)


def test_refusal_table_and_bound_are_exercised():
    """The cases reach both sides of the bound and both answers: some call above LSN_DCN_KD_EVERY_ROUTE is served, some refused
    for its LDS need, and the routes named in the issue's case table are the ones the cases file expects."""
    bound = ks.kd_every_route()
    above = [n for n in ks.NAMES if bound < ks.kd(ks.case(n)) <= 64]
    assert above == ['k8_bound', 'k4_dg4_bound']
    for n in above:
        assert ('LDS' in {v for (c, _, _), v in ks.EXPECTED_REFUSALS.items() if c == n})
        assert (n, 'default', 'bwd') not in ks.EXPECTED_REFUSALS and (n, 'default', 'fwd') not in ks.EXPECTED_REFUSALS
    assert ks.ROUTES['k1_one_chunk']['default'][0] == 'FWD_MM' and ks.ROUTES['k1_wgmm']['default'][2] == 'WG_MM'
    assert ks.ROUTES['k5_dg2']['default'][0] in ('FWD_XN', 'FWD_XN_PLANES', 'FWD_FP32')
    assert ks.ROUTES['k5_g8']['default'][0] == 'FWD_GROUPED' and ks.ROUTES['k5_g8']['default'][2] == 'WG_XN_ORDERED'
    assert ks.ROUTES['k2_g8']['default'][2] == 'WG_GROUPED'


# ------------------------------------------------------------------------------------------------------ anchor lists
@pytest.mark.parametrize('name', ['k1_one_chunk', 'k5_pyr', 'k5_dg2'])
def test_anchor_lists(name):
    """Sample ids pixel * KD + group * K + tap, list order and {samples, anchors} at KD = 1, 25 and 50."""
    c = ks.case(name)
    (x, w, b, off, mask, go, cfg), _, _ = ks.reference(name)
    with _kernel_choice('default'):
        launch = Launch([dict(x=x, off=off, mask=mask, scale=(cfg['sh'], cfg['sw']))], w.shape[0], groups=cfg['groups'], dg=cfg['dg'],
                        stride=cfg['stride'], pad=cfg['pad'], dil=cfg['dil'], k=c['k'])
        assert launch.ws_bytes > 0 and launch.prepared_ok() == 1      # GATHER_MM (ROUTES)
        anchor, start, sample, na = launch.lists()
        B, _, H, W = x.shape
        Ho, Wo = cfg['out_hw']
        assert na == B * (H + 1) * (W + 1) and anchor.numel() == B * Ho * Wo * ks.kd(c)
        listed = check_lists(anchor, start, sample, na)
        assert 0 < listed < anchor.numel()
        assert torch.equal(anchor, expected_anchor(launch, [off], dg=cfg['dg'], stride=cfg['stride'], pad=cfg['pad'], dil=cfg['dil'],
                                                   k=c['k']))


# ------------------------------------------------------------------------------------------------------ named entry points
@pytest.mark.parametrize('k', [(1, 3), (3, 1)], ids=['1x3', '3x1'])
def test_reference_named_entry_points_non_square(k):
    """The eight lsn_*deform_conv* wrappers (contiguous NCHW, the reference's argument order: W before H for v1 / pyramid, H
    before W for the modulated op) with a non-square kernel.  Stride / pad / dilation are equal per axis (the wrappers require
    it), so only the kernel's two extents tell the axes apart: swapped, the offset tensor has the wrong number of rows and
    columns for the output, or the values differ.  The pyramid wrappers demand an offset grid that the convolution arithmetic
    maps to itself (pyramid_shape_check of the reference); for a 1x3 kernel that leaves stride 2, pad 1 and a 3 x 1 grid."""
    lib = _lib.load()
    dev = _dev()
    kh, kw = k
    g = torch.Generator().manual_seed(21)
    B, C, Co, H, W = 2, 32, 48, 11, 13
    K = kh * kw
    Ho, Wo = orc.out_size(H, kh, 1, 1, 1), orc.out_size(W, kw, 1, 1, 1)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, kh, kw, generator=g) * (1.0 / (K * C) ** 0.5)
    b = torch.randn(Co, generator=g)
    off = torch.rand(B, 2 * K, Ho, Wo, generator=g) * 6 - 3
    mask = torch.rand(B, K, Ho, Wo, generator=g)
    go = torch.randn(B, Co, Ho, Wo, generator=g)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    one = ctypes.c_float(1.0)
    xd, wd, bd, od, md, gd = [t.to(dev).contiguous() for t in (x, w, b, off, mask, go)]
    errs = {}
    # modulated: kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w
    out = torch.empty(B, Co, Ho, Wo, device=dev)
    _lib.check(lib.lsn_modulated_deform_conv_forward(p(xd), p(wd), p(bd), p(od), p(md), p(out), B, C, H, W, Co, kh, kw, 1, 1, 1, 1, 1, 1,
                                                     1, 1, 1, st))
    errs['mdcn_fwd'] = _report('mdcn_fwd', out, orc.deform_conv_forward(x, w, b, off, mask, 1, 1, 1))
    gx, gw, gb, goff, gm = (torch.empty_like(t) for t in (xd, wd, bd, od, md))
    _lib.check(lib.lsn_modulated_deform_conv_backward(p(xd), p(wd), p(bd), p(od), p(md), p(gx), p(gw), p(gb), p(goff), p(gm), p(gd), B, C,
                                                      H, W, Co, kh, kw, 1, 1, 1, 1, 1, 1, 1, 1, 1, st))
    gref = orc.deform_conv_backward(x, w, off, mask, go, 1, 1, 1)
    for n, t in (('gx', gx), ('gw', gw), ('gb', gb), ('goff', goff), ('gmask', gm)):
        errs['mdcn_' + n] = _report('mdcn_' + n, t, gref[n])
    # v1: kW, kH, dW, dH, padW, padH, dilW, dilH
    out1 = torch.empty(B, Co, Ho, Wo, device=dev)
    _lib.check(lib.lsn_deform_conv_forward(p(xd), p(wd), p(od), p(out1), B, C, H, W, Co, kw, kh, 1, 1, 1, 1, 1, 1, 1, 1, B, st))
    errs['dcn1_fwd'] = _report('dcn1_fwd', out1, orc.deform_conv_forward(x, w, None, off, None, 1, 1, 1))
    g1 = orc.deform_conv_backward(x, w, off, None, go, 1, 1, 1)
    gx, gw, goff = (torch.empty_like(t) for t in (xd, wd, od))
    _lib.check(lib.lsn_deform_conv_backward_input(p(xd), p(od), p(gd), p(gx), p(goff), p(wd), B, C, H, W, Co, kw, kh, 1, 1, 1, 1, 1, 1, 1,
                                                  1, B, st))
    _lib.check(lib.lsn_deform_conv_backward_parameters(p(xd), p(od), p(gd), p(gw), B, C, H, W, Co, kw, kh, 1, 1, 1, 1, 1, 1, 1, 1, one,
                                                       B, st))
    for n, t in (('gx', gx), ('goff', goff), ('gw', gw)):
        errs['dcn1_' + n] = _report('dcn1_' + n, t, g1[n])
    # pyramid: Ho, Wo, kW, kH, dW, dH, padW, padH, dilW, dilH, scaleW, scaleH.  Stride 2, pad 1: a grid of 3 along the
    # kernel's extent-1 axis ((3 + 2 - 1) / 2 + 1 = 3) and of 1 along its extent-3 axis ((1 + 2 - 3) / 2 + 1 = 1)
    Hp, Wp = (3, 1) if k == (1, 3) else (1, 3)
    assert (orc.out_size(Hp, kh, 2, 1, 1), orc.out_size(Wp, kw, 2, 1, 1)) == (Hp, Wp)
    offp = torch.rand(B, 2 * K, Hp, Wp, generator=g) * 6 - 3
    gop = torch.randn(B, Co, Hp, Wp, generator=g)
    sh, sw = ctypes.c_float(H / Hp).value, ctypes.c_float(W / Wp).value      # (as the float arguments carry them)
    offpd, gopd = offp.to(dev), gop.to(dev)
    outp = torch.empty(B, Co, Hp, Wp, device=dev)
    _lib.check(lib.lsn_pyramid_deform_conv_forward(p(xd), p(wd), p(offpd), p(outp), B, C, H, W, Co, Hp, Wp, kw, kh, 2, 2, 1, 1, 1, 1,
                                                   ctypes.c_float(sw), ctypes.c_float(sh), 1, 1, B, st))
    errs['pyr_fwd'] = _report('pyr_fwd', outp, orc.deform_conv_forward(x, w, None, offp, None, 2, 1, 1, 1, 1, sh, sw, out_hw=(Hp, Wp)))
    gp = orc.deform_conv_backward(x, w, offp, None, gop, 2, 1, 1, 1, 1, sh, sw)
    gx, gw, goffp = torch.empty_like(xd), torch.empty_like(wd), torch.empty_like(offpd)
    _lib.check(lib.lsn_pyramid_deform_conv_backward_input(p(xd), p(offpd), p(gopd), p(gx), p(goffp), p(wd), B, C, H, W, Co, Hp, Wp, kw,
                                                          kh, 2, 2, 1, 1, 1, 1, ctypes.c_float(sw), ctypes.c_float(sh), 1, 1, B, st))
    _lib.check(lib.lsn_pyramid_deform_conv_backward_parameters(p(xd), p(offpd), p(gopd), p(gw), B, C, H, W, Co, Hp, Wp, kw, kh, 2, 2, 1,
                                                               1, 1, 1, ctypes.c_float(sw), ctypes.c_float(sh), 1, 1, one, B, st))
    torch.cuda.synchronize()
    for n, t in (('gx', gx), ('goff', goffp), ('gw', gw)):
        errs['pyr_' + n] = _report('pyr_' + n, t, gp[n])
    print('ENTRY', k, {n: f'{v:.1e}' for n, v in errs.items()})
    assert all(e < TOL for e in errs.values()), errs
