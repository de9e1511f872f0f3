"""The element arithmetic of the point-decoding kernels (lsnet_amd/csrc/point_rows.h, shared with csrc/points.hip) against the
torch statements of LSHead on the CPU, without a GPU: the header is compiled here with g++ under a loop-nest driver that states
every operation the way the kernels do, one output element at a time.

Everything behind the softplus is compared with torch.equal, from the header's own sp: the signed selection, the gradient_mul
mix with its separately rounded products, the base grid, the backward's scatter and gm products, the boxes and their
point + box * stride.  The softplus and its derivative are compared with float64 within 4 ulp, with an absolute floor of
2^-126.  That bound is derived, not measured: expf is at most 1 ulp off, log1p carries it on with an amplification of at most
1 and adds at most 2 ulp of its own (the OpenCL bound the device's math library follows), the final rounding adds 0.5; the
derivative z / (z + 1) stays below it (1 ulp of expf, two roundings).  The test prints what it reads: the header 1.48 ulp, its
derivative 2.34 ulp, torch's own CPU softplus 1.36 ulp on these inputs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import point_decode_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = r'''
#include <stddef.h>
#include "point_rows.h"

extern "C" void softplus_rows(const float *x, float *y, float *dy, long long n) {
    for (long long i = 0; i < n; ++i) y[i] = point_softplus(x[i]), dy[i] = point_softplus_grad(1.0f, x[i]);
}

extern "C" float one_minus(double gm) { return point_one_minus(gm); }

// sp = softplus(raw[:n_sp]); off from THAT sp (src: the offset table)
extern "C" void decode_fwd(const float *raw, long long rows, int c_raw, int n_sp, const int *src, int n_off, double gm64,
                           const float *base, float *sp, float *off) {
    const float om = point_one_minus(gm64), gm = (float)gm64;
    for (long long r = 0; r < rows; ++r) {
        const float *x = raw + r * c_raw;
        float *s = sp + r * n_sp;
        for (int c = 0; c < n_sp; ++c) s[c] = point_softplus(x[c]);
        for (int j = 0; j < n_off; ++j) {
            const float v = src[j] >= 0 ? point_signed(s[src[j]], s[src[j] + 1]) : x[n_sp + point_free_index(src[j])];
            off[r * n_off + j] = point_offset(v, gm, om, base[j]);
        }
    }
}

// the gradient that reaches sp (before the softplus derivative) and the free channels, one output element at a time
extern "C" void decode_bwd(const float *sp, const float *g_sp, const float *g_off, long long rows, int c_raw, int n_sp,
                           const int *src, int n_off, double gm64, float *g_pre, float *g_free) {
    const float gm = (float)gm64;
    for (long long r = 0; r < rows; ++r) {
        for (int c = 0; c < c_raw; ++c) {
            int j = -1;
            for (int k = 0; k < n_off; ++k)
                if (c < n_sp ? (src[k] >= 0 && src[k] == (c & ~1)) : (src[k] < 0 && n_sp + point_free_index(src[k]) == c)) j = k;
            if (c >= n_sp) {
                g_free[r * (c_raw - n_sp) + c - n_sp] = j >= 0 ? point_offset_grad(g_off[r * n_off + j], gm) : 0.f;
                continue;
            }
            float g = g_sp ? g_sp[r * n_sp + c] : 0.f;
            if (j >= 0) {
                const float *pair = sp + r * n_sp + (c & ~1);
                g = g + point_signed_grad(point_offset_grad(g_off[r * n_off + j], gm), pair[0], pair[1], c & 1);
            }
            g_pre[r * n_sp + c] = g;
        }
    }
}

extern "C" void boxes(const float *rows, int B, int n_all, int C, const float *points, int mode, int nv, float *out) {
    for (long long r = 0; r < (long long)B * n_all; ++r) {
        const float *p = rows + r * C, *pt = points + (r % n_all) * 3;
        float x0, y0, x1, y1;
        if (mode == POINT_BOX_EXTREME) {
            float y[4], x[4];
            for (int v = 0; v < 4; ++v) point_vector_yx(p + 4 * v, &y[v], &x[v]);
            x0 = x[1], y0 = y[0], x1 = x[3], y1 = y[2];
        } else {
            x0 = y0 = INFINITY, x1 = y1 = -INFINITY;
            for (int v = 0; v < nv; ++v) {
                float y, x;
                point_vector_yx(p + 4 * v, &y, &x);
                x0 = point_min(x0, x), y0 = point_min(y0, y), x1 = point_max(x1, x), y1 = point_max(y1, y);
            }
        }
        float *o = out + r * 4;
        o[0] = point_box_coord(pt[0], x0, pt[2]), o[1] = point_box_coord(pt[1], y0, pt[2]);
        o[2] = point_box_coord(pt[0], x1, pt[2]), o[3] = point_box_coord(pt[1], y1, pt[2]);
    }
}
'''

F32 = ctypes.POINTER(ctypes.c_float)
I32 = ctypes.POINTER(ctypes.c_int)
ULP_BOUND = 4.0


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp('points')
    src = d / 'driver.cpp'
    src.write_text(DRIVER)
    so = d / 'points.so'
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off',
                           f'-I{os.path.join(ROOT, "lsnet_amd", "csrc")}', str(src), '-o', str(so)])
    lib = ctypes.CDLL(str(so))
    lib.one_minus.restype = ctypes.c_float
    lib.one_minus.argtypes = [ctypes.c_double]
    return lib


def _a(t):
    return np.array(t.detach().numpy(), dtype=np.float32, order='C', copy=True)


def _p(a):
    return None if a is None else a.ctypes.data_as(F32)


def _table(c):
    from lsnet_amd.ops.point_decode import offset_sources
    src = offset_sources(c['task'], c['n_sp'], c['c_raw'], 9)
    return src, np.asarray(src, dtype=np.int32)


def _decode_fwd(lib, c):
    raw = _a(c['raw'])
    R = raw.shape[0] * raw.shape[1]
    src, tab = _table(c)
    sp, off = np.empty((pc.B, pc.N_ALL, c['n_sp']), np.float32), np.empty((pc.B, pc.N_ALL, len(src)), np.float32)
    base = _a(pc.base_offset().float())
    lib.decode_fwd(_p(raw), ctypes.c_longlong(R), c['c_raw'], c['n_sp'], tab.ctypes.data_as(I32), len(src), ctypes.c_double(pc.GM),
                   _p(base), _p(sp), _p(off))
    return torch.from_numpy(sp), torch.from_numpy(off)


def test_one_minus_gm_is_the_python_scalar_rounded(rows):
    for gm in (0.1, 0.3, 0.5, 0.7, 1.0, 0.0, 1e-3):
        assert rows.one_minus(gm) == float(torch.tensor(1 - gm, dtype=torch.float32))


@pytest.mark.parametrize('name', sorted(pc.LAYOUTS))
def test_offsets_from_the_headers_own_sp_equal_the_torch_statements(rows, name):
    c = pc.case(name)
    sp, off = _decode_fwd(rows, c)
    want = pc.offsets_from_sp(c, pc.px(sp), pc.px(c['raw']))
    assert off.shape[2] == 18 and torch.equal(pc.px(off), want)
    # the mix is not the identity: a kernel that shortcuts or contracts it is caught by the comparison above
    plain = pc.offsets_from_sp(c, pc.px(sp), pc.px(c['raw']), gm=1.0)
    assert (plain != want).float().mean() > 0.1
    # the planted ties are ties of sp as well, some of them at exactly 0
    assert torch.equal(sp[0, 0, 0::2], sp[0, 0, 1::2]) and torch.equal(sp[0, 3], torch.zeros_like(sp[0, 3]))


@pytest.mark.parametrize('name', sorted(pc.LAYOUTS))
def test_backward_scatter_and_gm_products_equal_autograd(rows, name):
    c = pc.case(name)
    sp, _ = _decode_fwd(rows, c)
    src, tab = _table(c)
    n_sp, c_raw = c['n_sp'], c['c_raw']
    R = pc.B * pc.N_ALL
    sp_leaf = pc.px(sp).clone().requires_grad_()
    raw_leaf = pc.px(c['raw']).clone().requires_grad_()
    off = pc.offsets_from_sp(c, sp_leaf, raw_leaf)
    for g_sp in (c['g_sp'], None):
        outs, grads = [off], [pc.px(c['g_off'])]
        if g_sp is not None:
            outs.append(sp_leaf * 1.0)
            grads.append(pc.px(g_sp))
        want_sp, want_raw = torch.autograd.grad(outs, [sp_leaf, raw_leaf], grads, retain_graph=True, allow_unused=True)
        g_pre = np.full((pc.B, pc.N_ALL, n_sp), np.nan, np.float32)
        g_free = np.full((pc.B, pc.N_ALL, max(c_raw - n_sp, 1)), np.nan, np.float32)
        rows.decode_bwd(_p(_a(sp)), _p(None if g_sp is None else _a(g_sp)), _p(_a(c['g_off'])), ctypes.c_longlong(R), c_raw, n_sp,
                        tab.ctypes.data_as(I32), len(src), ctypes.c_double(pc.GM), _p(g_pre), _p(g_free))
        assert torch.equal(pc.px(torch.from_numpy(g_pre)), want_sp)
        if c_raw > n_sp:
            assert torch.equal(pc.px(torch.from_numpy(g_free)), want_raw[:, n_sp:])
    # a tie sends the gradient to neg, negated (row 0 is all ties)
    j0 = src[0]
    assert g_pre[0, 0, j0] == -np.float32(np.float32(pc.GM) * c['g_off'][0, 0, 0].numpy()) and g_pre[0, 0, j0 + 1] == 0


@pytest.mark.parametrize('name', sorted(pc.LAYOUTS))
def test_boxes_equal_the_torch_statements(rows, name):
    c = pc.case(name)
    sp, _ = _decode_fwd(rows, c)
    pts = pc.flat_points()
    mode, nv = pc.box_mode(c)
    out = np.empty((pc.B, pc.N_ALL, 4), np.float32)
    rows.boxes(_p(_a(sp)), pc.B, pc.N_ALL, c['n_sp'], _p(_a(pts)), 0 if mode == 'extreme' else 1, nv, _p(out))
    want = pc.boxes_from_sp(c, pc.px(sp), pts)
    assert torch.equal(torch.from_numpy(out), want)
    from lsnet_amd.ops.point_decode import point_boxes
    assert torch.equal(point_boxes(sp, pts, mode, nv), want)          # (host tensors: the module's torch statements)


@pytest.mark.parametrize('nv,kind,task', [(4, 'bbox', 'bbox'), (36, 'segm', 'segm'), (17, 'pose', 'pose_kbox')])
def test_pick_tables_name_the_channels_get_pred_reg_reads(nv, kind, task):
    from lsnet_amd.models.dense_heads.ls_head import LSHead
    from lsnet_amd.ops.point_decode import offset_sources, point_decode
    n_sp = 4 * (nv + 1)
    c_raw = n_sp + 8 if kind == 'bbox' else n_sp
    src = offset_sources(task, n_sp, c_raw, 9)
    picks = pc.expected_picks(nv, kind)
    assert list(src[:2 * len(picks)]) == [4 * v + 2 * comp for v in picks for comp in (0, 1)]
    assert list(src[2 * len(picks):]) == [-1 - i for i in range(c_raw - n_sp)] and len(src) == 18
    # a sp whose value encodes its channel: pos wins with value c + 1, then neg wins with value 1000 - c
    chan = torch.arange(c_raw, dtype=torch.float32).view(1, -1, 1, 1)
    for sp, read in ((chan[:, :n_sp] + 1, lambda v: v - 2), (1000 - chan[:, :n_sp], lambda v: 1000 + v)):
        reg = LSHead.get_pred_reg(pc.stub(task, nv), sp, (2000 + chan[:, n_sp:]) if c_raw > n_sp else None)
        got = [int(read(v)) if v < 1500 else -1 - int(v - 2000 - n_sp) for v in reg.view(-1).tolist()]
        assert got == list(src)
    # the module's torch statements for a table are the head's statements
    c = dict(task=task, nv=nv, n_sp=n_sp)
    raw = 4 * torch.randn(2, c_raw, 5, 1, generator=pc.gen(3))
    sp, off = point_decode(raw, n_sp, src, pc.GM, pc.base_offset())
    want_sp, want_off = pc.head_statements(c, raw)
    assert torch.equal(sp, want_sp) and torch.equal(off, want_off)


def test_softplus_and_its_derivative_against_float64(rows):
    xs = torch.cat([pc.case(n)['raw'].reshape(-1) for n in sorted(pc.LAYOUTS)] +
                   [torch.linspace(-110, 30, 20001), torch.tensor(pc.EDGES), torch.tensor([0.0, -0.0, 19.999998, 88.0, -87.5, -103.9])])
    x = _a(xs)
    y, dy = np.empty_like(x), np.empty_like(x)
    rows.softplus_rows(_p(x), _p(y), _p(dy), ctypes.c_longlong(x.size))
    y, dy = torch.from_numpy(y), torch.from_numpy(dy)
    err = pc.ulp_error(y, pc.softplus64(xs)).max().item()
    err_d = pc.ulp_error(dy, pc.softplus_grad64(xs)).max().item()
    err_t = pc.ulp_error(torch.nn.functional.softplus(xs), pc.softplus64(xs)).max().item()
    print(f'POINTS host softplus {err:.2f} ulp, derivative {err_d:.2f} ulp, torch CPU softplus {err_t:.2f} ulp')
    assert err <= ULP_BOUND and err_d <= ULP_BOUND
    big = xs > 20
    assert torch.equal(y[big], xs[big]) and torch.equal(dy[big], torch.ones_like(xs[big]))
    assert y[xs == 20.0].eq(20.0).all() and (y[xs == -110.0] == 0).all()
