"""The index, tie and divisor arithmetic of the pooling kernels (lsnet_amd/csrc/pool_rows.h, shared with csrc/pool.hip) against
torch on the CPU, without a GPU: the header is compiled here with g++ under a loop-nest driver that states every operation the
way the kernels do -- one output (or, in the backwards, one input) element at a time, gathering in a fixed order.

Inputs are relu(randn) (about half zeros, so ties are the common case), gradients small integers, average-pool inputs small
integers as well: every sum is then exact in fp32 whatever its order, and every comparison below is torch.equal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = r'''
#include <math.h>
#include <stddef.h>
#include "pool_rows.h"

// channels-last: element (b, y, x, c) of a (B, h, w, C) map
static inline size_t at(int b, int y, int x, int c, int h, int w, int C) { return (((size_t)b * h + y) * w + x) * C + c; }

extern "C" int out_size(int in, int k, int s, int p, int ceil_mode) { return pool_out_size(in, k, s, p, ceil_mode); }

extern "C" void max_fwd(const float *x, float *y, unsigned char *slot, int B, int H, int W, int C, int kh, int kw, int s, int p) {
    const int Ho = pool_out_size(H, kh, s, p, 0), Wo = pool_out_size(W, kw, s, p, 0);
    for (int b = 0; b < B; ++b) for (int oh = 0; oh < Ho; ++oh) for (int ow = 0; ow < Wo; ++ow) for (int c = 0; c < C; ++c) {
        const int h0 = oh * s - p, w0 = ow * s - p;
        const int ilo = h0 < 0 ? -h0 : 0, ihi = h0 + kh > H ? H - h0 : kh, jlo = w0 < 0 ? -w0 : 0, jhi = w0 + kw > W ? W - w0 : kw;
        float best = -INFINITY;
        int win = ilo * kw + jlo;
        for (int i = ilo; i < ihi; ++i) for (int j = jlo; j < jhi; ++j) {
            const float v = x[at(b, h0 + i, w0 + j, c, H, W, C)];
            if (pool_max_takes(v, best)) best = v, win = i * kw + j;
        }
        y[at(b, oh, ow, c, Ho, Wo, C)] = best;
        slot[at(b, oh, ow, c, Ho, Wo, C)] = (unsigned char)win;
    }
}

extern "C" void max_bwd(const float *gy, const unsigned char *slot, float *gx, int B, int H, int W, int C, int kh, int kw, int s, int p) {
    const int Ho = pool_out_size(H, kh, s, p, 0), Wo = pool_out_size(W, kw, s, p, 0);
    for (int b = 0; b < B; ++b) for (int ih = 0; ih < H; ++ih) for (int iw = 0; iw < W; ++iw) for (int c = 0; c < C; ++c) {
        int olo, ohi, plo, phi;
        pool_cover(ih, kh, s, p, Ho, &olo, &ohi);
        pool_cover(iw, kw, s, p, Wo, &plo, &phi);
        float acc = 0.f;
        for (int oh = olo; oh <= ohi; ++oh) for (int ow = plo; ow <= phi; ++ow) {
            const int mine = (ih - (oh * s - p)) * kw + (iw - (ow * s - p));
            if (!slot || slot[at(b, oh, ow, c, Ho, Wo, C)] == mine) acc += gy[at(b, oh, ow, c, Ho, Wo, C)];
        }
        gx[at(b, ih, iw, c, H, W, C)] = acc;
    }
}

extern "C" void avg_fwd(const float *x, float *y, int *divisor, int B, int H, int W, int C, int kh, int kw, int s, int p, int ceil_mode,
                        int cip) {
    const int Ho = pool_out_size(H, kh, s, p, ceil_mode), Wo = pool_out_size(W, kw, s, p, ceil_mode);
    for (int b = 0; b < B; ++b) for (int oh = 0; oh < Ho; ++oh) for (int ow = 0; ow < Wo; ++ow) {
        int hlo, hhi, hext, wlo, whi, wext;
        pool_window(oh, kh, s, p, H, &hlo, &hhi, &hext);
        pool_window(ow, kw, s, p, W, &wlo, &whi, &wext);
        const int div = pool_avg_divisor(hlo, hhi, hext, wlo, whi, wext, cip);
        if (b == 0) divisor[oh * Wo + ow] = div;
        for (int c = 0; c < C; ++c) {
            float sum = 0.f;
            for (int ih = hlo; ih < hhi; ++ih) for (int iw = wlo; iw < whi; ++iw) sum += x[at(b, ih, iw, c, H, W, C)];
            y[at(b, oh, ow, c, Ho, Wo, C)] = (hlo < hhi && wlo < whi) ? sum / (float)div : sum;
        }
    }
}

extern "C" void avg_bwd(const float *gy, float *gx, int B, int H, int W, int C, int kh, int kw, int s, int p, int ceil_mode, int cip) {
    const int Ho = pool_out_size(H, kh, s, p, ceil_mode), Wo = pool_out_size(W, kw, s, p, ceil_mode);
    for (int b = 0; b < B; ++b) for (int ih = 0; ih < H; ++ih) for (int iw = 0; iw < W; ++iw) for (int c = 0; c < C; ++c) {
        int olo, ohi, plo, phi;
        pool_cover(ih, kh, s, p, Ho, &olo, &ohi);
        pool_cover(iw, kw, s, p, Wo, &plo, &phi);
        float acc = 0.f;
        for (int oh = olo; oh <= ohi; ++oh) for (int ow = plo; ow <= phi; ++ow) {
            int hlo, hhi, hext, wlo, whi, wext;
            pool_window(oh, kh, s, p, H, &hlo, &hhi, &hext);
            pool_window(ow, kw, s, p, W, &wlo, &whi, &wext);
            acc += gy[at(b, oh, ow, c, Ho, Wo, C)] / (float)pool_avg_divisor(hlo, hhi, hext, wlo, whi, wext, cip);
        }
        gx[at(b, ih, iw, c, H, W, C)] = acc;
    }
}

extern "C" int up_ok(int small, int big) { return pool_up_ok(small, big); }
extern "C" void up_src(int n, long long *src) { for (int i = 0; i < n; ++i) src[i] = pool_up_src(i); }

extern "C" void up_add_fwd(const float *top, const float *lat, float *out, int B, int h, int w, int H, int W, int C) {
    for (int b = 0; b < B; ++b) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) for (int c = 0; c < C; ++c)
        out[at(b, y, x, c, H, W, C)] = lat[at(b, y, x, c, H, W, C)] + top[at(b, pool_up_src(y), pool_up_src(x), c, h, w, C)];
}

extern "C" void up_add_bwd(const float *go, float *gt, int accumulate, int B, int h, int w, int H, int W, int C) {
    for (int b = 0; b < B; ++b) for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) for (int c = 0; c < C; ++c) {
        const bool right = 2 * x + 1 < W, down = 2 * y + 1 < H;
        float acc = go[at(b, 2 * y, 2 * x, c, H, W, C)];
        if (right) acc += go[at(b, 2 * y, 2 * x + 1, c, H, W, C)];
        if (down) acc += go[at(b, 2 * y + 1, 2 * x, c, H, W, C)];
        if (right && down) acc += go[at(b, 2 * y + 1, 2 * x + 1, c, H, W, C)];
        float *dst = gt + at(b, y, x, c, h, w, C);
        *dst = accumulate ? *dst + acc : acc;
    }
}

// element of scan step t of line l
static inline size_t line_at(int mode, int b, int l, int t, int c, int H, int W, int C) {
    const int n = pool_corner_along_x(mode) ? W : H, p = pool_corner_pos(mode, t, n);
    return pool_corner_along_x(mode) ? at(b, l, p, c, H, W, C) : at(b, p, l, c, H, W, C);
}

extern "C" void corner_fwd(int mode, const float *x, float *y, int accumulate, int B, int H, int W, int C) {
    const int lines = pool_corner_along_x(mode) ? H : W, n = pool_corner_along_x(mode) ? W : H;
    for (int b = 0; b < B; ++b) for (int l = 0; l < lines; ++l) for (int c = 0; c < C; ++c) {
        float best = x[line_at(mode, b, l, 0, c, H, W, C)];
        for (int t = 0; t < n; ++t) {
            const float v = x[line_at(mode, b, l, t, c, H, W, C)];
            if (pool_corner_takes(v, best)) best = v;
            float *dst = y + line_at(mode, b, l, t, c, H, W, C);
            *dst = accumulate ? *dst + best : best;
        }
    }
}

extern "C" void corner_bwd(int mode, const float *x, const float *gy, float *gx, int accumulate, int B, int H, int W, int C) {
    const int lines = pool_corner_along_x(mode) ? H : W, n = pool_corner_along_x(mode) ? W : H;
    for (int b = 0; b < B; ++b) for (int l = 0; l < lines; ++l) for (int c = 0; c < C; ++c) {
        float best = x[line_at(mode, b, l, 0, c, H, W, C)], acc = 0.f;
        int pos = 0;
        for (int t = 0; t < n; ++t) {
            const float v = x[line_at(mode, b, l, t, c, H, W, C)], d = gy[line_at(mode, b, l, t, c, H, W, C)];
            if (pool_corner_takes(v, best)) {
                if (t > 0) {
                    float *dst = gx + line_at(mode, b, l, pos, c, H, W, C);
                    *dst = accumulate ? *dst + acc : acc;
                }
                best = v, pos = t, acc = d;
            } else {
                acc += d;
                if (!accumulate) gx[line_at(mode, b, l, t, c, H, W, C)] = 0.f;
            }
        }
        float *dst = gx + line_at(mode, b, l, pos, c, H, W, C);
        *dst = accumulate ? *dst + acc : acc;
    }
}
'''

F32 = ctypes.POINTER(ctypes.c_float)
MODES = {'top': 0, 'bottom': 1, 'left': 2, 'right': 3}
DIM_FLIP = {'bottom': (2, False), 'left': (3, True), 'right': (3, False), 'top': (2, True)}
AVG_CFGS = [(3, 2, 1, False, True), (2, 2, 0, True, False)]      # Res2Net: the pooled scale, the avg_down shortcut
SIZES = [(13, 17), (14, 18), (25, 42), (1, 1)]


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp('pool')
    src = d / 'driver.cpp'
    src.write_text(DRIVER)
    so = d / 'pool.so'
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off',
                           f'-I{os.path.join(ROOT, "lsnet_amd", "csrc")}', str(src), '-o', str(so)])
    return ctypes.CDLL(str(so))


def _nhwc(t):
    """(B, C, H, W) tensor -> dense (B, H, W, C) float32 array of its own (never a view of the tensor)"""
    return np.array(t.detach().permute(0, 2, 3, 1).numpy(), dtype=np.float32, order='C', copy=True)


def _nchw(a):
    return torch.from_numpy(a).permute(0, 3, 1, 2)


def _p(a):
    return a.ctypes.data_as(F32)


def _relu_randn(seed, *shape):
    x = torch.relu(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)))
    assert (x == 0).float().mean() > 0.3, 'ties must really be present'
    return x


def _ints(seed, *shape):
    return torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(seed)).float()


def _same(got, want):
    """torch.equal with NaNs at the same places"""
    return got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want)) and \
        torch.equal(torch.nan_to_num(got, nan=0.), torch.nan_to_num(want, nan=0.))


def run_max(lib, x, k, s, p, go=None):
    B, C, H, W = x.shape
    Ho, Wo = lib.out_size(H, k, s, p, 0), lib.out_size(W, k, s, p, 0)
    xa = _nhwc(x)
    y, slot = np.empty((B, Ho, Wo, C), np.float32), np.empty((B, Ho, Wo, C), np.uint8)
    lib.max_fwd(_p(xa), _p(y), slot.ctypes.data_as(ctypes.c_void_p), B, H, W, C, k, k, s, p)
    gx = None
    if go is not None:
        gx = np.empty((B, H, W, C), np.float32)
        lib.max_bwd(_p(_nhwc(go)), slot.ctypes.data_as(ctypes.c_void_p) if k > 1 else None, _p(gx), B, H, W, C, k, k, s, p)
        gx = _nchw(gx)
    return _nchw(y), torch.from_numpy(slot.astype(np.int64)).permute(0, 3, 1, 2), gx


def _slot_to_index(slot, k, s, p, W):
    """the flat input index ATen's return_indices reports for a winning window position"""
    B, C, Ho, Wo = slot.shape
    oh = torch.arange(Ho).view(1, 1, Ho, 1)
    ow = torch.arange(Wo).view(1, 1, 1, Wo)
    return (oh * s - p + slot // k) * W + (ow * s - p + slot % k)


@pytest.mark.parametrize('k,s,p', [(3, 2, 1), (1, 2, 0)])
@pytest.mark.parametrize('hw', [(13, 17), (14, 18), (25, 42), (1, 1), (5, 5)])
def test_max_pool(rows, k, s, p, hw):
    x = _relu_randn(1, 2, 8, *hw).requires_grad_()
    want, idx = F.max_pool2d(x, k, s, p, return_indices=True)
    go = _ints(2, *want.shape)
    (gwant,) = torch.autograd.grad(want, x, go)
    y, slot, gx = run_max(rows, x, k, s, p, go)
    assert torch.equal(y, want)
    assert torch.equal(_slot_to_index(slot, k, s, p, hw[1]), idx)
    assert torch.equal(gx, gwant)


def test_max_pool_first_maximum_wins_on_a_zero_map(rows):
    _, slot, _ = run_max(rows, torch.zeros(1, 4, 5, 5), 3, 2, 1)
    idx = _slot_to_index(slot, 3, 2, 1, 5)
    assert idx[0, 0].flatten().tolist() == [0, 1, 3, 5, 6, 8, 15, 16, 18]
    assert torch.equal(idx, F.max_pool2d(torch.zeros(1, 4, 5, 5), 3, 2, 1, return_indices=True)[1])


@pytest.mark.parametrize('special', ['inf', 'nan'])
def test_max_pool_inf_and_nan(rows, special):
    x = _relu_randn(3, 2, 4, 13, 17)
    if special == 'inf':
        x[0, 0, 3, 4], x[0, 1, 6, 6], x[1, 2, 0, 0] = float('inf'), float('-inf'), float('inf')
        x[1, 3, :5, :5] = float('-inf')              # whole windows of -inf
    else:
        x[0, 0, 3, 4], x[1, 2, 12, 16], x[1, 1, 0, 0] = float('nan'), float('nan'), float('nan')
    x.requires_grad_()
    want, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    go = _ints(4, *want.shape)
    (gwant,) = torch.autograd.grad(want, x, go)
    y, slot, gx = run_max(rows, x, 3, 2, 1, go)
    assert _same(y, want) and torch.isnan(y).any() == (special == 'nan')
    assert torch.equal(_slot_to_index(slot, 3, 2, 1, 17), idx)
    assert torch.equal(gx, gwant)


@pytest.mark.parametrize('cfg', AVG_CFGS, ids=['3-2-1', '2-2-0-ceil'])
@pytest.mark.parametrize('hw', SIZES)
def test_avg_pool(rows, cfg, hw):
    k, s, p, ceil_mode, cip = cfg
    H, W = hw
    x = _ints(5, 2, 8, H, W).requires_grad_()
    want = F.avg_pool2d(x, k, s, p, ceil_mode, cip)
    Ho, Wo = rows.out_size(H, k, s, p, int(ceil_mode)), rows.out_size(W, k, s, p, int(ceil_mode))
    assert (Ho, Wo) == tuple(want.shape[2:])
    go = _ints(6, *want.shape)
    (gwant,) = torch.autograd.grad(want, x, go)
    y, div = np.empty((2, Ho, Wo, 8), np.float32), np.empty((Ho, Wo), np.int32)
    rows.avg_fwd(_p(_nhwc(x)), _p(y), div.ctypes.data_as(ctypes.c_void_p), 2, H, W, 8, k, k, s, p, int(ceil_mode), int(cip))
    # the divisor: what the framework divides a map of ones by
    ones = F.avg_pool2d(torch.ones(1, 1, H, W), k, s, p, ceil_mode, cip, divisor_override=1)
    frac = F.avg_pool2d(torch.ones(1, 1, H, W), k, s, p, ceil_mode, cip)
    assert torch.equal(ones[0, 0] / torch.from_numpy(div).float(), frac[0, 0])
    assert torch.equal(_nchw(y), want)
    gx = np.empty((2, H, W, 8), np.float32)
    rows.avg_bwd(_p(_nhwc(go)), _p(gx), 2, H, W, 8, k, k, s, p, int(ceil_mode), int(cip))
    assert torch.equal(_nchw(gx), gwant)


def test_upsample_indices_are_nearest_interpolation(rows):
    """index halving == F.interpolate(mode='nearest') for every h in 1 .. 1024 and both output sizes"""
    src = np.empty(2048, np.int64)
    rows.up_src(2048, src.ctypes.data_as(ctypes.c_void_p))
    src = torch.from_numpy(src)
    for h in range(1, 1025):
        ramp = torch.arange(h, dtype=torch.float32).view(1, 1, h, 1)
        for H in (2 * h, 2 * h - 1):
            assert rows.up_ok(h, H)
            want = F.interpolate(ramp, size=(H, 1), mode='nearest').flatten().long()
            assert torch.equal(src[:H], want), (h, H)
    for h, H in ((4, 9), (4, 6), (4, 4), (1, 3), (0, 0), (3, 8)):
        assert not rows.up_ok(h, H)


@pytest.mark.parametrize('hw,HW', [((13, 21), (25, 42)), ((25, 42), (50, 84)), ((25, 42), (50, 83)), ((25, 42), (49, 84)),
                                   ((1, 1), (1, 1)), ((1, 1), (2, 2))])
def test_upsample_add(rows, hw, HW):
    (h, w), (H, W) = hw, HW
    top = _ints(7, 2, 8, h, w).requires_grad_()
    lat = _ints(8, 2, 8, H, W).requires_grad_()
    want = lat + F.interpolate(top, size=(H, W), mode='nearest')
    go = _ints(9, 2, 8, H, W)
    gt_want, gl_want = torch.autograd.grad(want, [top, lat], go)
    out = np.empty((2, H, W, 8), np.float32)
    rows.up_add_fwd(_p(_nhwc(top)), _p(_nhwc(lat)), _p(out), 2, h, w, H, W, 8)
    assert torch.equal(_nchw(out), want) and torch.equal(gl_want, go)
    gt = np.empty((2, h, w, 8), np.float32)
    rows.up_add_bwd(_p(_nhwc(go)), _p(gt), 0, 2, h, w, H, W, 8)
    assert torch.equal(_nchw(gt), gt_want)
    base = _ints(10, 2, 8, h, w)
    gt = _nhwc(base)
    rows.up_add_bwd(_p(_nhwc(go)), _p(gt), 1, 2, h, w, H, W, 8)
    assert torch.equal(_nchw(gt), base + gt_want)


def _cummax_pool(x, mode):
    dim, flip = DIM_FLIP[mode]
    if flip:
        x = x.flip(dim)
    out = torch.cummax(x, dim=dim)[0]
    return out.flip(dim) if flip else out


def run_corner(lib, mode, x, go, accumulate_onto=None):
    B, C, H, W = x.shape
    xa = _nhwc(x)
    y = np.zeros((B, H, W, C), np.float32) if accumulate_onto is None else _nhwc(accumulate_onto[0])
    lib.corner_fwd(MODES[mode], _p(xa), _p(y), int(accumulate_onto is not None), B, H, W, C)
    gx = np.zeros((B, H, W, C), np.float32) if accumulate_onto is None else _nhwc(accumulate_onto[1])
    lib.corner_bwd(MODES[mode], _p(xa), _p(_nhwc(go)), _p(gx), int(accumulate_onto is not None), B, H, W, C)
    return _nchw(y), _nchw(gx)


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('hw', [(13, 21), (7, 11), (1, 5), (5, 1), (1, 1)])
def test_corner_pool(rows, mode, hw):
    x = (_relu_randn(11, 2, 8, 13, 21)[:, :, :hw[0], :hw[1]]).clone().requires_grad_()
    want = _cummax_pool(x, mode)
    go = _ints(12, *x.shape)
    (gwant,) = torch.autograd.grad(want, x, go)
    y, gx = run_corner(rows, mode, x, go)
    assert torch.equal(y, want) and torch.equal(gx, gwant)
    base_y, base_g = _ints(13, *x.shape), _ints(14, *x.shape)
    y, gx = run_corner(rows, mode, x, go, accumulate_onto=(base_y, base_g))
    assert torch.equal(y, base_y + want.detach()) and torch.equal(gx, base_g + gwant)


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('special', ['inf', 'nan'])
def test_corner_pool_inf_and_nan(rows, mode, special):
    x = _relu_randn(15, 2, 4, 13, 21)
    if special == 'inf':
        x[0, 0, 6, 10], x[0, 1, 0, 0], x[1, 2, 12, 20] = float('inf'), float('-inf'), float('-inf')
        x[1, 3, 4, :], x[1, 3, :, 7] = float('-inf'), float('-inf')
    else:
        x[0, 0, 6, 10], x[0, 0, 6, 15], x[0, 0, 2, 10], x[1, 2, 0, 0], x[1, 1, 12, 20] = (float('nan'),) * 5
    x.requires_grad_()
    want = _cummax_pool(x, mode)
    go = _ints(16, *x.shape)
    (gwant,) = torch.autograd.grad(want, x, go)
    y, gx = run_corner(rows, mode, x, go)
    assert _same(y, want) and torch.isnan(y).any() == (special == 'nan')
    assert torch.equal(gx, gwant)


def test_exports_of_the_pooling_family():
    """The loader lists the new entry points, the built library exports them, and they validate before any device work."""
    from lsnet_amd import _lib
    from lsnet_amd.csrc import build
    names = ['lsn_pool_output_size', 'lsn_max_pool2d_forward', 'lsn_max_pool2d_backward', 'lsn_avg_pool2d_forward',
             'lsn_avg_pool2d_backward', 'lsn_upsample_add_forward', 'lsn_upsample_add_backward', 'lsn_corner_pool_forward',
             'lsn_corner_pool_backward']
    assert set(names) <= set(_lib.EXPORTS)
    lib = ctypes.CDLL(build.build())
    for n in names:
        assert hasattr(lib, n), n
    lib = _lib.load()
    assert [lib.lsn_pool_output_size(n, 3, 2, 1, 0) for n in (400, 239, 1)] == [200, 120, 1]
    assert [lib.lsn_pool_output_size(n, 2, 2, 0, 1) for n in (13, 14, 1)] == [7, 7, 1]
    assert lib.lsn_pool_output_size(2, 3, 1, 0, 0) == 0
    a = ctypes.c_void_p(1 << 20)          # never dereferenced: the calls below are refused before any launch
    assert lib.lsn_max_pool2d_forward(a, 6, a, 6, None, 1, 8, 8, 6, 3, 3, 2, 1, None) == -1
    assert b'not a multiple of 4' in lib.lsn_last_error()
    assert lib.lsn_avg_pool2d_forward(a, 10, a, 8, 1, 8, 8, 8, 3, 3, 2, 1, 0, 1, None) == -1
    assert b'pixel pitch of x is 10' in lib.lsn_last_error()
    assert lib.lsn_avg_pool2d_backward(ctypes.c_void_p((1 << 20) + 4), 8, a, 8, 1, 8, 8, 8, 3, 3, 2, 1, 0, 1, None) == -1
    assert b'not 16-byte aligned' in lib.lsn_last_error()
    assert lib.lsn_upsample_add_forward(a, 8, a, 8, a, 8, 1, 4, 4, 9, 8, 8, None) == -1
    assert b'is not a doubling' in lib.lsn_last_error()
    assert lib.lsn_upsample_add_backward(a, 8, a, 8, 0, 1, 4, 4, 6, 8, 8, None) == -1
    assert lib.lsn_corner_pool_forward(4, a, 8, a, 8, 0, 1, 8, 8, 8, None) == -1
    assert b'mode 4' in lib.lsn_last_error()
    assert lib.lsn_corner_pool_backward(0, a, 8, a, 8, a, 8, 0, 1, 8, 8, 8, None) == -1
    assert lib.lsn_max_pool2d_backward(a, 8, None, a, 8, 1, 8, 8, 8, 3, 3, 2, 1, None) == -1
    assert b'needs the slots' in lib.lsn_last_error()
