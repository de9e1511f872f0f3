"""The polygon / keypoint stage rows of lsnet_amd/csrc/cross_iou_row.h (the text the device kernel of csrc/loss.hip runs on its
LDS tile), compiled here with g++, against the float64 statement of LSHead.loss_levels + cross_iou_loss and its autograd
gradient at the inputs of tests/loss_stage_cases.py; and the argument checks of lsn_cross_iou_stage_forward / _backward
through the C ABI of the built library, which need no GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import loss_edge_cases as lec
from tests import loss_stage_cases as lsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = r'''
#include "cross_iou_row.h"
// in_place: the gradient is written over a copy of the prediction row, as the device kernel does on its tile
extern "C" void stage_rows(int kind, const float *raw, const float *pts, const float *anchor3, const float *box, const float *vs,
                           const unsigned char *obj, int n, int nv, int sub, float base, float alpha, float eps, int in_place,
                           float *loss, float *grad) {
    const int M = 4 * (nv + 1);
    for (int i = 0; i < n; ++i) {
        float *g = grad + M * i;
        const float *p = raw + M * i;
        if (in_place) {
            for (int c = 0; c < M; ++c) g[c] = p[c];
            p = g;
        }
        loss[i] = kind == 1 ? cross_iou_polygon_stage_row(p, pts + M / 2 * i, anchor3 + 3 * i, box + 4 * i, obj[i], base, nv, sub,
                                                          alpha, eps, g)
                            : cross_iou_keypoint_stage_row(p, pts + M / 2 * i, anchor3 + 3 * i, vs + nv * i, obj[i], base, nv, alpha,
                                                           eps, g);
    }
}
// the device kernel's order of work: lay the values of the row down first (pn over the gradient row, dn in `scratch`), walk
// the prepared row with the gradient written over pn, take it through ciou_stage_grad
extern "C" void stage_rows_prepared(int kind, const float *raw, const float *pts, const float *anchor3, const float *box,
                                    const float *vs, const unsigned char *obj, int n, int nv, int sub, float base, float alpha,
                                    float eps, float *scratch, float *loss, float *grad) {
    const int M = 4 * (nv + 1);
    for (int i = 0; i < n; ++i) {
        const float *a3 = anchor3 + 3 * i;
        const float stride = a3[2], norm = base * stride;
        float *g = grad + M * i;
        for (int c = 0; c < M; ++c) g[c] = ciou_stage_p(raw[M * i + c], stride, norm);
        for (int j = 0; j < M / 2; ++j) scratch[j] = ciou_stage_d(pts[M / 2 * i + j], a3[j & 1], obj[i], norm);
        loss[i] = kind == 1 ? cross_iou_polygon_stage_row_prepared(g, scratch, a3, box + 4 * i, base, nv, sub, alpha, eps, g)
                            : cross_iou_keypoint_stage_row_prepared(g, scratch, vs + nv * i, nv, alpha, eps, g);
        for (int c = 0; c < M; ++c) g[c] = ciou_stage_grad(g[c], stride, norm);
    }
}
extern "C" void stage_loss_only(int kind, const float *raw, const float *pts, const float *anchor3, const float *box,
                                const float *vs, const unsigned char *obj, int n, int nv, int sub, float base, float alpha,
                                float eps, float *loss) {
    const int M = 4 * (nv + 1);
    for (int i = 0; i < n; ++i)
        loss[i] = kind == 1 ? cross_iou_polygon_stage_row(raw + M * i, pts + M / 2 * i, anchor3 + 3 * i, box + 4 * i, obj[i], base,
                                                          nv, sub, alpha, eps, nullptr)
                            : cross_iou_keypoint_stage_row(raw + M * i, pts + M / 2 * i, anchor3 + 3 * i, vs + nv * i, obj[i], base,
                                                           nv, alpha, eps, nullptr);
}
'''


@pytest.fixture(scope='module')
def rowlib(tmp_path_factory):
    d = tmp_path_factory.mktemp('ciou_stage')
    src = d / 'driver.cpp'
    src.write_text(DRIVER)
    so = d / 'ciou_stage.so'
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off',
                           f'-I{os.path.join(ROOT, "lsnet_amd", "csrc")}', str(src), '-o', str(so)])
    return ctypes.CDLL(str(so))


def _host_rows(rowlib, kind, case, nv, sub, alpha, in_place):
    n, m = case['raw'].shape
    f32, u8 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_ubyte)
    arrs = [np.ascontiguousarray(case[k].numpy(), dtype=np.float32) for k in ('raw', 'gt_pts', 'anchor3', 'box', 'vs')]
    obj = np.ascontiguousarray((case['weight'] > 0).numpy().astype(np.uint8))
    loss, only, grad = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, m), np.float32)
    k = 1 if kind == 'polygon' else 2
    head = [k] + [a.ctypes.data_as(f32) for a in arrs] + [obj.ctypes.data_as(u8), n, nv, sub, ctypes.c_float(lec.BASE_SCALE),
                                                           ctypes.c_float(alpha), ctypes.c_float(1e-6)]
    rowlib.stage_rows(*head, int(in_place), loss.ctypes.data_as(f32), grad.ctypes.data_as(f32))
    rowlib.stage_loss_only(*head, only.ctypes.data_as(f32))
    assert np.array_equal(loss, only)                                 # the loss does not depend on the gradient request
    if in_place:                                                      # ... nor on the values having been laid down before
        loss_p, grad_p, scratch = np.zeros(n, np.float32), np.zeros((n, m), np.float32), np.zeros(m // 2, np.float32)
        rowlib.stage_rows_prepared(*head, scratch.ctypes.data_as(f32), loss_p.ctypes.data_as(f32), grad_p.ctypes.data_as(f32))
        assert np.array_equal(loss, loss_p) and np.array_equal(grad, grad_p)
    return loss, grad


@pytest.mark.parametrize('alpha', lsc.ALPHAS)
@pytest.mark.parametrize('kind,nv,sub', lsc.CASES)
def test_stage_rows_match_the_head_formulation(rowlib, kind, nv, sub, alpha):
    case = lsc.shared_case(kind, nv, sub)
    ref, gref = lsc.reference(kind, nv, sub, alpha)
    assert torch.isfinite(ref).all() and torch.isfinite(gref).all()              # every row, none masked out
    assert lec.decisions_agree(case['raw'], *lsc.stage_targets(case, torch.float32), alpha)
    dead = case['weight'] == 0
    assert dead.sum() >= 500 and not ref[dead].any() and not gref[dead].any()
    loss, grad = _host_rows(rowlib, kind, case, nv, sub, alpha, in_place=False)
    loss_i, grad_i = _host_rows(rowlib, kind, case, nv, sub, alpha, in_place=True)
    assert np.array_equal(loss, loss_i) and np.array_equal(grad, grad_i)        # gradient written over the prediction: same bits
    w, up = case['weight'].numpy(), case['up'].numpy()
    np.testing.assert_allclose(loss * w, ref.numpy(), rtol=5e-5, atol=5e-6)
    got, want = grad.astype(np.float64) * (up * w)[:, None], gref.numpy()
    scale = np.abs(want).max(1, keepdims=True) + 1e-6
    err = float((np.abs(got - want) / scale).max())
    print(f'{kind} nv {nv} sub {sub} alpha {alpha}: loss {float(np.abs(loss * w - ref.numpy()).max()):.2e}  grad {err:.2e}')
    assert err < 5e-4, err
    assert not got[dead.numpy()].any()


def test_the_cases_hold_what_they_promise():
    case = lsc.shared_case('polygon', 36, 9)
    a = case['anchor3']
    obj = case['weight'] > 0
    assert torch.equal(a[:, :2] / a[:, 2:3], (a[:, :2] / a[:, 2:3]).round())     # anchors: integer multiples of the stride
    off = (case['gt_pts'] - a[:, :2].repeat(1, 37)) / a[:, 2:3]
    assert torch.equal(off[obj] * 64, (off[obj] * 64).round()) and float(off[obj].abs().max()) <= 3
    assert float(off[1, 0]) == 0.0 and bool(obj[1])
    assert not case['gt_pts'][~obj].any() and not case['box'][~obj].any() and 500 <= int((~obj).sum()) <= 700
    target, active = lsc.stage_targets(case, torch.float32)
    ties = (case['raw'] == target) & active
    assert ties[0::7].sum() > 100 and not ties[1::7].sum() > ties[0::7].sum()
    assert set(case['vs'].unique().tolist()) == {0.0, 2.0}


def _stage_call(lib, which, kind, ncomp, sub, box=0x1000, vs=0x1000, n=3):
    """a call with plausible non-null addresses: refused before any device work, so nothing reads them"""
    a = 0x1000
    if which == 'forward':
        return lib.lsn_cross_iou_stage_forward(kind, a, a, a, box, vs, a, n, ncomp, sub, 4.0, 0.2, 1e-6, a, None)
    return lib.lsn_cross_iou_stage_backward(kind, a, a, a, box, vs, a, a, n, ncomp, sub, 4.0, 0.2, 1e-6, a, None)


@pytest.mark.parametrize('which', ['forward', 'backward'])
def test_stage_argument_checks_need_no_gpu(which):
    from lsnet_amd import _lib
    from lsnet_amd.csrc import build
    build.build()
    lib = _lib.load()
    who = f'lsn_cross_iou_stage_{which}'.encode()
    rc = _stage_call(lib, which, 1, 10, 9)
    assert rc == -1 and who + b': rows have 4 (nv + 1) components, got 10' in lib.lsn_last_error()
    rc = _stage_call(lib, which, 1, 4, 1)
    assert rc == -1 and who + b': rows have 4 (nv + 1) components, got 4' in lib.lsn_last_error()
    for sub in (0, 17):
        rc = _stage_call(lib, which, 1, 148, sub)
        assert rc == -1 and who + f': subset stride {sub} out of range'.encode() in lib.lsn_last_error()
    rc = _stage_call(lib, which, 1, 16, 5)                                         # more subsets than landmarks
    assert rc == -1 and who + b': subset stride 5 out of range' in lib.lsn_last_error()
    rc = _stage_call(lib, which, 1, 148, 9, box=None)
    assert rc == -1 and who + b': the polygon loss needs anchor points and ground-truth boxes' in lib.lsn_last_error()
    rc = _stage_call(lib, which, 2, 72, 9, vs=None)
    assert rc == -1 and who + b': the keypoint loss needs the visibility values' in lib.lsn_last_error()
    rc = _stage_call(lib, which, 3, 72, 9)
    assert rc == -1 and who + b': kind must be 1 (polygon) or 2 (keypoint), got 3' in lib.lsn_last_error()
    rc = _stage_call(lib, which, 2, 72, 9, n=-1)
    assert rc == -1 and who + b': invalid number of rows -1' in lib.lsn_last_error()
    # the tile of 64 rows has to fit 64 KiB of LDS: polygon up to 164 components, keypoint (with its visibilities) up to 140
    for kind, ncomp in ((1, 168), (2, 144)):
        rc = _stage_call(lib, which, kind, ncomp, 9)
        assert rc not in (0, -1) and who + f': rows of {ncomp} components need'.encode() in lib.lsn_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(rc)
