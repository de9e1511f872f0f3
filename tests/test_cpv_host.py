"""The element arithmetic of the corner-verification kernels (lsnet_amd/csrc/cpv_rows.h, shared with csrc/cpv.hip) against the
torch statements, without a GPU: the header is compiled here with g++ under a loop-nest driver that states the targets the
way the kernels do -- per (gt, corner, level) the packed minimum of (distance bits, row) into a small table, per (corner,
point) the Gaussian maximum over the gts and the last gt of the table that took the point -- and the three losses element by
element with double sums.  Inputs and their near-tie condition: tests/cpv_cases.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lsnet_amd.models.losses import GaussianFocalLoss, SEPFocalLoss, SmoothL1Loss
from tests import cpv_cases as cc
from tests import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = r'''
#include <vector>
#include "cpv_rows.h"

extern "C" void targets(const float *pts, int P, const unsigned char *valid, const float *gt, int G, int bump, double iou,
                        float *hm, float *off, int *npos) {
    const cpv_radius_consts rk = cpv_radius_constants(iou);
    std::vector<int> win((size_t)G * 2 * CPV_LEVELS, -1);
    std::vector<float> rs((size_t)G * 2);
    for (int g = 0; g < G; ++g) {
        const float *box = gt + 4 * g;
        rs[2 * g] = bump ? cpv_gaussian_radius(box[3] - box[1], box[2] - box[0], rk) : 0.f;
        rs[2 * g + 1] = bump ? cpv_sigma(rs[2 * g]) : 1.f;
        for (int c = 0; c < 2; ++c)
            for (int lev = 0; lev < CPV_LEVELS; ++lev) {
                unsigned long long best = ~0ull;
                for (int i = 0; i < P; ++i) {
                    if (valid && !valid[i]) continue;
                    if (assign_point_level(pts[3 * i + 2]) != lev) continue;
                    const uint32_t key = assign_key(cpv_corner_distance(pts[3 * i], pts[3 * i + 1], box[2 * c], box[2 * c + 1]));
                    if (key >= 0xff800000u) continue;
                    const unsigned long long cand = ((unsigned long long)key << 32) | (unsigned)i;
                    best = cand < best ? cand : best;
                }
                win[((size_t)g * 2 + c) * CPV_LEVELS + lev] = best == ~0ull ? -1 : (int)(best & 0xffffffffu);
            }
    }
    for (int c = 0; c < 2; ++c) {
        npos[c] = 0;
        for (int p = 0; p < P; ++p) {
            float h = 0.f, ox = 0.f, oy = 0.f;
            if (!valid || valid[p]) {
                const int lev = assign_point_level(pts[3 * p + 2]);
                const bool on = lev >= 0 && lev < CPV_LEVELS;
                int winner = -1;
                for (int g = 0; g < G; ++g) {
                    if (bump)
                        h = fmaxf(h, cpv_heat(cpv_corner_distance(pts[3 * p], pts[3 * p + 1], gt[4 * g + 2 * c], gt[4 * g + 2 * c + 1]),
                                              rs[2 * g], rs[2 * g + 1]));
                    if (on && win[((size_t)g * 2 + c) * CPV_LEVELS + lev] == p) winner = g;
                }
                if (winner >= 0) {
                    h = 1.f;
                    ox = cpv_offset(gt[4 * winner + 2 * c], pts[3 * p], lev);
                    oy = cpv_offset(gt[4 * winner + 2 * c + 1], pts[3 * p + 1], lev);
                }
            }
            hm[(size_t)c * P + p] = h;
            off[((size_t)c * P + p) * 2] = ox, off[((size_t)c * P + p) * 2 + 1] = oy;
        }
        // the positives as the kernel counts them: the distinct rows of the table
        for (int g = 0; g < G; ++g)
            for (int lev = 0; lev < CPV_LEVELS; ++lev) {
                const int row = win[((size_t)g * 2 + c) * CPV_LEVELS + lev];
                if (row < 0) continue;
                bool later = false;
                for (int q = g + 1; q < G && !later; ++q) later = win[((size_t)q * 2 + c) * CPV_LEVELS + lev] == row;
                npos[c] += later ? 0 : 1;
            }
    }
}

// sum_i w_i loss(x_i, t_i) in double, and the derivative of every element with respect to its logit
extern "C" double gaussian_focal(int n, const float *x, const float *t, const float *w, float alpha, float gamma, float *dx) {
    double s = 0.;
    for (int i = 0; i < n; ++i) {
        float d;
        const float v = cpv_gaussian_focal(x[i], t[i], alpha, gamma, &d);
        if (w[i] != 0.f) s += (double)v;
        dx[i] = w[i] != 0.f ? d : 0.f;
    }
    return s;
}

extern "C" double smooth_l1(int n, const float *pred, const float *target, const float *w, float beta, float *dp) {
    double s = 0.;
    for (int i = 0; i < n; ++i) {
        float d;
        const float v = cpv_smooth_l1(pred[i], target[i], beta, &d);
        if (w[i] != 0.f) s += (double)v;
        dp[i] = w[i] != 0.f ? d : 0.f;
    }
    return s;
}

// the SEP focal loss of n elements as the finishing kernel forms it; dx: the gradient of the loss
extern "C" float sep_focal(int n, const float *x, const float *t, const float *w, float gamma, float alpha, float *dx) {
    double s[5] = {0., 0., 0., 0., 0.};
    for (int i = 0; i < n; ++i) {
        if (t[i] == 1.f) s[0] += (double)cpv_sep_focal_pos(x[i], w[i], gamma, alpha, nullptr), s[1] += (double)w[i], s[3] += 1.;
        else if (t[i] < 1.f) s[2] += (double)cpv_sep_focal_neg(x[i], gamma, alpha, nullptr);
        if (t[i] > 0.f) s[4] += 1.;
    }
    const float wsum = (float)s[1], avg = (float)s[4];
    const float gpos = s[3] > 0. ? 1.f / wsum : 0.f, gneg = 1.f / avg;
    for (int i = 0; i < n; ++i) {
        float d = 0.f;
        dx[i] = 0.f;
        if (t[i] == 1.f) cpv_sep_focal_pos(x[i], w[i], gamma, alpha, &d), dx[i] = gpos * d;
        else if (t[i] < 1.f) cpv_sep_focal_neg(x[i], gamma, alpha, &d), dx[i] = gneg * d;
    }
    return (s[3] > 0. ? (float)s[0] / wsum : 0.f) + (float)s[2] / avg;
}

extern "C" int nearest_index(int dst, int in, int out) { return cpv_nearest_index(dst, in, out); }
'''

F32, I32, U8 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_ubyte)


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp('cpv')
    src = d / 'driver.cpp'
    src.write_text(DRIVER)
    so = d / 'cpv.so'
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off',
                           f'-I{os.path.join(ROOT, "lsnet_amd", "csrc")}', str(src), '-o', str(so)])
    lib = ctypes.CDLL(str(so))
    lib.gaussian_focal.restype = lib.smooth_l1.restype = ctypes.c_double
    lib.sep_focal.restype = ctypes.c_float
    return lib


def _f(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)


def run_targets(lib, pts, valid, boxes, bump, iou=0.7):
    """-> hm (2, P), off (2, P, 2), npos (2,) as torch tensors"""
    p, g = _f(pts), _f(boxes)
    P = len(p)
    v = None if valid is None else np.ascontiguousarray(valid.numpy(), dtype=np.uint8)
    hm, off, npos = np.zeros((2, P), np.float32), np.zeros((2, P, 2), np.float32), np.zeros(2, np.int32)
    lib.targets(p.ctypes.data_as(F32), P, None if v is None else v.ctypes.data_as(U8), g.ctypes.data_as(F32), len(g), int(bump),
                ctypes.c_double(iou), hm.ctypes.data_as(F32), off.ctypes.data_as(F32), npos.ctypes.data_as(I32))
    return torch.from_numpy(hm), torch.from_numpy(off), torch.from_numpy(npos)


@pytest.mark.parametrize('case', cc.all_cases(), ids=lambda c: c[0])
def test_targets_match_the_torch_statement(rows, case):
    name, hw, boxes = case
    pts = cc.grid(hw)
    valid = cc.valid_mask(len(pts))
    for mask in (None, valid):
        sub = pts if mask is None else pts[mask]
        assert cc.margins_ok(sub, boxes), 'a near-tie in the inputs: replace the case in cpv_cases.CASES'
        for bump in (True, False):
            want = cc.statement(pts, mask, boxes, bump)
            assert (want[0] == 1).any()
            cc.same_targets(run_targets(rows, pts, mask, boxes, bump), want, (name, mask is not None, bump))
    if name == 'large_boxes':
        bumps = ((want_b := cc.statement(pts, None, boxes, True)[0]) > 0) & (want_b < 1)
        assert bumps.sum(1).tolist() == [46, 30] and (want_b == 1).sum(1).tolist() == [15, 17]


def test_targets_match_the_reference_fixture(rows):
    """tests/golden/cpv_assigner.npz is the reference's own PointHMAssigner on 384 x 512 points; tolerance of tests/test_cpv.py"""
    ref = np.load(os.path.join(ROOT, 'tests', 'golden', 'cpv_assigner.npz'))
    pts = cc.grid((384, 512))
    for seed, n in ((1, 5), (2, 9), (3, 1), (4, 30)):
        boxes = gu.make_gt(seed, n, 384, 512, num_classes=8)[0]
        for bump in (True, False):
            hm, off, npos = run_targets(rows, pts, None, boxes, bump)
            for c, base in ((0, 0), (1, 4)):
                want_hm, want_off, want_pos = (torch.from_numpy(ref[f'{seed}/{int(bump)}/{base + i}']) for i in range(3))
                assert torch.allclose(hm[c], want_hm.float(), rtol=1e-6, atol=1e-7), (seed, bump, c)
                assert torch.allclose(off[c], want_off, rtol=1e-6, atol=1e-7), (seed, bump, c)
                assert torch.equal(torch.nonzero(hm[c] == 1).squeeze(-1), want_pos) and int(npos[c]) == len(want_pos)
    keep = torch.rand(pts.shape[0], generator=gu.gen(0)) < 0.7      # the fixture's filtered point set, boxes of seed 4
    hm, off, _ = run_targets(rows, pts, keep, boxes, True)
    for c, base in ((0, 0), (1, 4)):
        assert torch.allclose(hm[c][keep], torch.from_numpy(ref[f'keep/{base}']), rtol=1e-6, atol=1e-7)
        assert torch.allclose(off[c][keep], torch.from_numpy(ref[f'keep/{base + 1}']), rtol=1e-6, atol=1e-7)
        assert not hm[c][~keep].any() and not off[c][~keep].any()


def _loss_inputs(seed, n=600):
    g = gu.gen(seed)
    x = torch.randn(n, generator=g) * 1.5
    t = torch.rand(n, generator=g) ** 3
    t[::11] = 1.0
    t[1::5] = 0.0
    w = (torch.rand(n, generator=g) > 0.25).float()
    return x, t, w


def test_gaussian_focal_and_smooth_l1_match_the_classes(rows):
    for seed, (alpha, gamma) in enumerate([(2.0, 4.0), (2.0, 4.0), (1.5, 3.0)]):
        x, t, w = _loss_inputs(seed)
        dx = np.zeros(len(x), np.float32)
        got = rows.gaussian_focal(len(x), _f(x).ctypes.data_as(F32), _f(t).ctypes.data_as(F32), _f(w).ctypes.data_as(F32),
                                  ctypes.c_float(alpha), ctypes.c_float(gamma), dx.ctypes.data_as(F32))
        arms = []
        for dt in (torch.float64, torch.float32):
            xx = x.to(dt).requires_grad_()
            loss = GaussianFocalLoss(alpha=alpha, gamma=gamma)(xx.sigmoid(), t.to(dt), w.to(dt), avg_factor=1.0)
            loss.backward()
            arms.append((loss.detach().double(), xx.grad.double()))
        cc.judge(torch.tensor(got), arms[1][0], arms[0][0], f'gaussian focal {seed}')
        cc.judge(torch.from_numpy(dx).double(), arms[1][1], arms[0][1], f'gaussian focal gradient {seed}')
    for seed, beta in enumerate([1.0 / 9.0, 1.0, 0.02]):
        g = gu.gen(20 + seed)
        a, b = torch.randn(400, generator=g) * 0.3, torch.randn(400, generator=g) * 0.3
        b[::9] = a[::9]                                            # d == 0
        a[1::9] = b[1::9] + beta                                   # (about) |d| == beta: the strict comparison
        w = (torch.rand(400, generator=g) > 0.3).float()
        dp = np.zeros(400, np.float32)
        got = rows.smooth_l1(400, _f(a).ctypes.data_as(F32), _f(b).ctypes.data_as(F32), _f(w).ctypes.data_as(F32),
                             ctypes.c_float(beta), dp.ctypes.data_as(F32))
        arms = []
        for dt in (torch.float64, torch.float32):
            aa = a.to(dt).requires_grad_()
            loss = SmoothL1Loss(beta=beta)(aa, b.to(dt), w.to(dt), avg_factor=1.0)
            loss.backward()
            arms.append((loss.detach().double(), aa.grad.double()))
        cc.judge(torch.tensor(got), arms[1][0], arms[0][0], f'smooth l1 {seed}')
        # |d| within an ulp of beta takes either branch in float64 and fp32: those elements are left to the value check
        edge = ((a - b).abs() - beta).abs() < 1e-6
        cc.judge(torch.from_numpy(dp).double()[~edge], arms[1][1][~edge], arms[0][1][~edge], f'smooth l1 gradient {seed}')


def test_sep_focal_matches_the_class(rows):
    for seed, (gamma, alpha, positives) in enumerate([(2.0, 0.25, True), (2.0, 0.25, False), (1.5, 0.4, True)]):
        g = gu.gen(40 + seed)
        x = torch.randn(700, generator=g) * 1.5
        t = (torch.rand(700, generator=g) > 0.8).float() if positives else torch.zeros(700)
        t[::13] = 0.5                                              # counted by target > 0, a negative of the loss
        w = torch.rand(700, generator=g) + 0.1
        dx = np.zeros(700, np.float32)
        got = rows.sep_focal(700, _f(x).ctypes.data_as(F32), _f(t).ctypes.data_as(F32), _f(w).ctypes.data_as(F32),
                             ctypes.c_float(gamma), ctypes.c_float(alpha), dx.ctypes.data_as(F32))
        arms = []
        for dt in (torch.float64, torch.float32):
            xx = x.to(dt).requires_grad_()
            loss = SEPFocalLoss(gamma=gamma, alpha=alpha)(xx, t.to(dt), w.to(dt), avg_factor=(t > 0).sum())
            loss.backward()
            arms.append((loss.detach().double(), xx.grad.double()))
        cc.judge(torch.tensor(float(got)).double(), arms[1][0], arms[0][0], f'sep focal {seed}')
        cc.judge(torch.from_numpy(dx).double(), arms[1][1], arms[0][1], f'sep focal gradient {seed}')


def test_nearest_index_is_interpolates(rows):
    """exact, for the semantic maps' sizes: 33x47 -> every level of both grids, 100x168 -> the levels of an 800 x 1344 image"""
    pairs = [((33, 47), s) for s in cc.level_sizes(cc.GRID_A) + cc.level_sizes(cc.GRID_B)] + \
            [((100, 168), s) for s in ((50, 84), (25, 42), (13, 21), (7, 11))]
    for (h, w), (H, W) in pairs:
        src = torch.arange(h * w, dtype=torch.float32).view(1, 1, h, w)
        want = F.interpolate(src, (H, W)).long()[0, 0]
        ys = torch.tensor([rows.nearest_index(y, h, H) for y in range(H)])
        xs = torch.tensor([rows.nearest_index(x, w, W) for x in range(W)])
        assert torch.equal(ys[:, None] * w + xs[None, :], want), ((h, w), (H, W))


def test_library_argument_checks_need_no_gpu():
    """The entry points validate before any device work: every refusal leaves a text and launches nothing."""
    from lsnet_amd import _lib
    lib = _lib.load()
    assert lib.lsn_corner_targets_workspace_bytes(300) >= 300 * (2 * 16 * 4 + 8)
    off = (ctypes.c_int * 2)(0, 3)
    assert lib.lsn_corner_targets_batch(None, 0, None, None, 1, off, 1, 0.7, None, None, None, None, None) == -1
    assert b'P = 0' in lib.lsn_last_error()
    many = (ctypes.c_int * 66)(*range(66))
    assert lib.lsn_corner_targets_batch(None, 10, None, None, 65, many, 1, 0.7, None, None, None, None, None) == -1
    assert b'65 images' in lib.lsn_last_error()
    lv = (_lib.CornerLevel * 9)()
    assert lib.lsn_corner_loss_forward(2, 9, 9, lv, None, None, None, None, 2.0, 4.0, 0.1, None, None, None, None) == -1
    assert b'9 levels' in lib.lsn_last_error()
    sv = (_lib.SemLevel * 9)()
    assert lib.lsn_sep_focal_forward(2, 3, 9, sv, None, None, 4, 4, 2.0, 0.25, None, None, None, None) == -1
    assert b'9 levels' in lib.lsn_last_error()
