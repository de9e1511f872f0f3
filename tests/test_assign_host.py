"""The row arithmetic of the assignment kernels (lsnet_amd/csrc/assign_rows.h, shared with csrc/assign.hip) against the torch
statements of core/assigners.py, without a GPU: the header is compiled here with g++ under a loop-nest driver that states both
assigners the way the kernels do -- per gt the k nearest rows of a segment (equal distances by ascending row), per row the
best gt that picked it (equal values to the lowest gt index).  Inputs and their near-tie condition: tests/assign_cases.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from lsnet_amd.core import ATSSAssigner, CentroidAssigner
from tests import assign_cases as ac
from tests import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = r'''
#include <vector>
#include "assign_rows.h"

// the k smallest (key, row) pairs of rows [start, start + n) that keyfn does not skip (0xffffffff), ascending
template <class F>
static std::vector<int> nearest(int start, int n, int k, F keyfn) {
    std::vector<int> out;
    unsigned long long last = 0;
    for (int r = 0; r < k; ++r) {
        unsigned long long best = ~0ull;
        for (int i = 0; i < n; ++i) {
            const uint32_t key = keyfn(start + i);
            if (key == 0xffffffffu) continue;
            const unsigned long long c = ((unsigned long long)key << 32) | (unsigned)i;
            if ((r == 0 || c > last) && c < best) best = c;
        }
        if (best == ~0ull) break;
        out.push_back(start + (int)(best & 0xffffffffu));
        last = best;
    }
    return out;
}

extern "C" void centroid(const float *pts, int P, const float *gt, const float *cen, int G, float scale, int pos_num,
                         const long long *gt_labels, long long *gt_inds, long long *labels) {
    std::vector<int> lvl(P);
    int lo = 1 << 30, hi = -(1 << 30);
    for (int i = 0; i < P; ++i) {
        lvl[i] = assign_point_level(pts[3 * i + 2]);
        lo = lvl[i] < lo ? lvl[i] : lo, hi = lvl[i] > hi ? lvl[i] : hi;
    }
    std::vector<uint32_t> best(P, 0xffffffffu);
    for (int i = 0; i < P; ++i) gt_inds[i] = 0;
    for (int g = 0; g < G; ++g) {
        const float *b = gt + 4 * g;
        const float w = assign_gt_extent(b[0], b[2]), h = assign_gt_extent(b[1], b[3]);
        const float cx = cen ? cen[2 * g] : assign_box_centre(b[0], b[2]), cy = cen ? cen[2 * g + 1] : assign_box_centre(b[1], b[3]);
        const int gl = assign_gt_level(w, h, scale, lo, hi);
        auto key = [&](int i) {
            return lvl[i] != gl ? 0xffffffffu : assign_key(assign_centroid_distance(pts[3 * i], pts[3 * i + 1], cx, cy, w, h));
        };
        for (int row : nearest(0, P, pos_num, key))
            if (key(row) < best[row]) best[row] = key(row), gt_inds[row] = g + 1;   // strict: the lowest gt index keeps a tie
    }
    if (labels)
        for (int i = 0; i < P; ++i) labels[i] = gt_inds[i] > 0 ? gt_labels[gt_inds[i] - 1] : -1;
}

extern "C" void atss(const float *boxes, int ld, int N, int nlev, const int *level_len, const float *gt, int G, int topk,
                     const long long *gt_labels, long long *gt_inds, float *max_overlaps, long long *labels) {
    for (int i = 0; i < N; ++i) gt_inds[i] = 0, max_overlaps[i] = -1e8f;
    for (int g = 0; g < G; ++g) {
        const float *b = gt + 4 * g;
        const float gx = assign_box_centre(b[0], b[2]), gy = assign_box_centre(b[1], b[3]);
        std::vector<int> cand;
        int start = 0;
        for (int l = 0; l < nlev; ++l) {
            auto key = [&](int i) {
                const float *q = boxes + (size_t)i * ld;
                return assign_key(assign_centre_distance(assign_box_centre(q[0], q[2]), assign_box_centre(q[1], q[3]), gx, gy));
            };
            for (int row : nearest(start, level_len[l], topk, key)) cand.push_back(row);
            start += level_len[l];
        }
        std::vector<float> iou;
        for (int row : cand) iou.push_back(assign_iou(boxes + (size_t)row * ld, b));
        const float thr = assign_atss_threshold(iou.data(), (int)iou.size());
        for (size_t c = 0; c < cand.size(); ++c) {
            const float *q = boxes + (size_t)cand[c] * ld;
            if (iou[c] >= thr && assign_centre_inside(assign_box_centre(q[0], q[2]), assign_box_centre(q[1], q[3]), b) &&
                iou[c] > max_overlaps[cand[c]])                                        // strict: the lowest gt index keeps a tie
                max_overlaps[cand[c]] = iou[c], gt_inds[cand[c]] = g + 1;
        }
    }
    if (labels)
        for (int i = 0; i < N; ++i) labels[i] = gt_inds[i] > 0 ? gt_labels[gt_inds[i] - 1] : -1;
}

extern "C" float key_roundtrip(float v) { return assign_key_value(assign_key(v)); }
'''

F32, I64, I32 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp('assign')
    src = d / 'driver.cpp'
    src.write_text(DRIVER)
    so = d / 'assign.so'
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off',
                           f'-I{os.path.join(ROOT, "lsnet_amd", "csrc")}', str(src), '-o', str(so)])
    lib = ctypes.CDLL(str(so))
    lib.key_roundtrip.restype = ctypes.c_float
    return lib


def _f(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)


def run_centroid(lib, pts, gt, centres, scale, pos_num, gt_labels):
    p, g = _f(pts), _f(gt)
    c = None if centres is None else _f(centres)
    lab = np.ascontiguousarray(gt_labels.numpy(), dtype=np.int64)
    gt_inds, labels = np.zeros(len(p), np.int64), np.zeros(len(p), np.int64)
    lib.centroid(p.ctypes.data_as(F32), len(p), g.ctypes.data_as(F32), None if c is None else c.ctypes.data_as(F32), len(g),
                 ctypes.c_float(scale), pos_num, lab.ctypes.data_as(I64), gt_inds.ctypes.data_as(I64), labels.ctypes.data_as(I64))
    return gt_inds, labels


def run_atss(lib, boxes, level_len, gt, topk, gt_labels):
    b, g = _f(boxes), _f(gt)
    lab = np.ascontiguousarray(gt_labels.numpy(), dtype=np.int64)
    lens = (ctypes.c_int * len(level_len))(*level_len)
    n = len(b)
    gt_inds, labels, mo = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float32)
    lib.atss(b.ctypes.data_as(F32), b.shape[1], n, len(level_len), lens, g.ctypes.data_as(F32), len(g), topk,
             lab.ctypes.data_as(I64), gt_inds.ctypes.data_as(I64), mo.ctypes.data_as(F32), labels.ctypes.data_as(I64))
    return gt_inds, mo, labels


def _centres(typ, b, e):
    return CentroidAssigner.gen_centroid(e, len(b)) if typ == 'centroid' else None


@pytest.mark.parametrize('case', ac.CASES, ids=lambda c: f'gt{c[0]}_G{c[1]}')
def test_driver_matches_the_torch_statements(rows, case):
    seed, ng, pseed, fixture_index, topks = case
    pts, sizes = ac.grid()
    b, l, e = gu.make_gt(seed, ng, 800, 800)
    props = ac.proposals(pts, pseed)
    assert ac.margins_ok(pts, sizes, b, e, props, topks), 'a near-tie in the inputs: replace the case in assign_cases.CASES'
    ref = np.load(os.path.join(ROOT, 'tests', 'golden', 'assign.npz'))
    for pos_num, typ in ac.CENTROID_MODES:
        want = CentroidAssigner(scale=4, pos_num=pos_num, iou_type=typ).assign(pts, b, e, None, l)
        got, labels = run_centroid(rows, pts, b, _centres(typ, b, e), 4, pos_num, l)
        assert (want.gt_inds > 0).any()
        assert np.array_equal(got, want.gt_inds.numpy()), (pos_num, typ)
        assert np.array_equal(labels, want.labels.numpy()), (pos_num, typ)
        key = {(1, 'center'): 'init', (3, 'centroid'): 'centroid'}.get((pos_num, typ))
        if fixture_index is not None and key is not None:
            assert np.array_equal(got, ref[f'{key}/{fixture_index}/gt_inds']), key
            if key == 'init':
                assert np.array_equal(labels, ref[f'init/{fixture_index}/labels'])
    level_len = [s[0] * s[1] for s in sizes]
    for topk in topks:
        want = ATSSAssigner(topk=topk).assign(props, level_len, b, None, l)
        got, mo, labels = run_atss(rows, props, level_len, b, topk, l)
        assert np.array_equal(got, want.gt_inds.numpy()), topk
        assert np.array_equal(labels, want.labels.numpy()), topk
        pos = got > 0
        assert pos.any() and np.array_equal(mo[pos], want.max_overlaps.numpy()[pos]), topk      # the same bits
        assert (mo[~pos] == np.float32(-1e8)).all()
        if fixture_index is not None and topk == 9:
            assert np.array_equal(got, ref[f'atss/{fixture_index}/gt_inds'])
            gu.check(f'atss/{fixture_index}/max_overlaps', torch.from_numpy(mo), ref, 1e-3, stride=5)


def test_constructed_ties(rows):
    pts, sizes = ac.grid()
    xy = {(int(x), int(y)): i for i, (x, y, s) in enumerate(pts.tolist()) if s == 8}
    for name, gts, pos_num, expect in ac.centroid_ties():
        want = np.zeros(len(pts), np.int64)
        for p, g in expect.items():
            want[xy[p]] = g
        lab = torch.arange(len(gts)) + 10
        got, labels = run_centroid(rows, pts, gts, None, 4, pos_num, lab)
        assert np.array_equal(got, want), name
        assert np.array_equal(labels, np.where(want > 0, want + 9, -1)), name
    boxes, level_len, topk, gts, want, iou = ac.atss_tie()
    for order in ([0, 1], [1, 0]):      # whichever of the mirror-image gts comes first keeps the shared box
        got, mo, _ = run_atss(rows, boxes, level_len, gts[order], topk, torch.tensor([3, 4]))
        assert got.tolist() == want and mo[2] == np.float32(iou)
        ref = ATSSAssigner(topk=topk).assign(boxes, level_len, gts[order], None, None)
        assert ref.gt_inds.tolist() == want and float(ref.max_overlaps[2]) == iou


def test_keys_order_like_floats(rows):
    vals = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 0.5, 1.0, 1e8, np.inf], np.float32)
    for v in vals:
        assert np.float32(rows.key_roundtrip(ctypes.c_float(v))) == v


def test_library_argument_checks_need_no_gpu():
    """The new entry points validate before any device work, like the rest of the C ABI."""
    from lsnet_amd import _lib
    lib = _lib.load()
    assert lib.lsn_assign_workspace_bytes(22400, 300, 5, 9) >= 22400 * 8 + 300 * 45 * 8
    assert lib.lsn_centroid_assign(None, 0, None, None, 3, ctypes.c_float(4), 1, None, None, None, None, None) == -1
    lens = (ctypes.c_int * 2)(100, 5)       # a level shorter than topk is refused (torch's topk raises there)
    assert lib.lsn_atss_assign(None, 4, 105, 2, lens, None, 3, 9, None, None, None, None, None, None) == -1
    assert b'level 1 has 5 boxes' in lib.lsn_last_error()
    assert lib.lsn_dense_targets(None, 5, None, 0, None, None) == -1
