"""The ragged-batch rules of the assignment kernels (lsnet_amd/csrc/assign_rows.h: which rows exist for an image, and the
label / weight / target rule of lsn_assign_targets_batch) without a GPU: the header is compiled with g++ under a loop-nest
driver that states the masked assigners and the target call the way the kernels do, and compared exactly with the torch
statements on the FILTERED points / boxes, scattered back (tests/assign_ragged_cases.py).  Also: what LSHead.get_points
caches for a ragged batch, and ATSSAssigner.assign_batch refusing a level with fewer than topk valid cells."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from lsnet_amd.core import ATSSAssigner, CentroidAssigner
from tests import assign_cases as ac
from tests import assign_ragged_cases as rc

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

// one image of a masked batch: valid = its row of the mask, or NULL
extern "C" void centroid(const float *pts, int P, const uint8_t *valid, const float *gt, const float *cen, int G, float scale,
                         int pos_num, const long long *gt_labels, long long *gt_inds, long long *labels) {
    std::vector<int> lvl(P);
    int lo = 1 << 30, hi = -(1 << 30);
    for (int i = 0; i < P; ++i) {                   // the range over ALL points, as the kernel takes it
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
            if (lvl[i] != gl || !assign_row_valid(valid, i)) return 0xffffffffu;
            return assign_key(assign_centroid_distance(pts[3 * i], pts[3 * i + 1], cx, cy, w, h));
        };
        for (int row : nearest(0, P, pos_num, key))
            if (key(row) < best[row]) best[row] = key(row), gt_inds[row] = g + 1;
    }
    if (labels)
        for (int i = 0; i < P; ++i) labels[i] = gt_inds[i] > 0 ? gt_labels[gt_inds[i] - 1] : -1;
}

extern "C" void atss(const float *boxes, int ld, int N, int nlev, const int *level_len, const uint8_t *valid, const float *gt,
                     int G, int topk, const long long *gt_labels, long long *gt_inds, float *max_overlaps, long long *labels) {
    for (int i = 0; i < N; ++i) gt_inds[i] = 0, max_overlaps[i] = -1e8f;
    for (int g = 0; g < G; ++g) {
        const float *b = gt + 4 * g;
        const float gx = assign_box_centre(b[0], b[2]), gy = assign_box_centre(b[1], b[3]);
        std::vector<int> cand;
        int start = 0;
        for (int l = 0; l < nlev; ++l) {
            auto key = [&](int i) {
                if (!assign_row_valid(valid, i)) return 0xffffffffu;
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
                iou[c] > max_overlaps[cand[c]])
                max_overlaps[cand[c]] = iou[c], gt_inds[cand[c]] = g + 1;
        }
    }
    if (labels)
        for (int i = 0; i < N; ++i) labels[i] = gt_inds[i] > 0 ? gt_labels[gt_inds[i] - 1] : -1;
}

extern "C" void targets(const long long *gt_inds, const uint8_t *valid, int P, int B, const int *off, const float *table, int D,
                        const long long *gt_labels, long long background, float *rows, long long *labels, float *label_weights,
                        float *bbox_weights, long long *num_pos) {
    for (int b = 0; b < B; ++b) {
        const int ng = off[b + 1] - off[b];
        num_pos[b] = 0;
        for (int i = 0; i < P; ++i) {
            const size_t p = (size_t)b * P + i;
            const int ok = assign_row_valid(valid, p), pos = assign_target_positive(gt_inds[p], ok, ng);
            num_pos[b] += pos;
            for (int d = 0; d < D; ++d) rows[p * D + d] = assign_target_value(pos, table + (size_t)off[b] * D, D, gt_inds[p], d);
            labels[p] = assign_target_label(pos, ok, gt_labels ? (const int64_t *)gt_labels + off[b] : 0, gt_inds[p], background);
            label_weights[p] = assign_target_label_weight(ok);
            for (int c = 0; c < 4; ++c) bbox_weights[p * 4 + c] = assign_target_bbox_weight(pos);
        }
    }
}
'''

F32, I64, U8 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp('assign_ragged')
    src = d / 'driver.cpp'
    src.write_text(DRIVER)
    so = d / 'assign_ragged.so'
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off',
                           f'-I{os.path.join(ROOT, "lsnet_amd", "csrc")}', str(src), '-o', str(so)])
    return ctypes.CDLL(str(so))


@pytest.fixture(scope='module')
def images():
    return {k: rc.image(k) for k in list(rc.IMAGES) + [None]}


def _f(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)


def _u8(flags):
    return None if flags is None else np.ascontiguousarray(flags.numpy(), dtype=np.uint8)


def _p(a, typ):
    return None if a is None else a.ctypes.data_as(typ)


def run_centroid(lib, pts, flags, gt, centres, pos_num, gt_labels):
    p, g, v = _f(pts), _f(gt), _u8(flags)
    c = None if centres is None else _f(centres)
    lab = None if gt_labels is None else np.ascontiguousarray(gt_labels.numpy(), dtype=np.int64)
    gt_inds = np.zeros(len(p), np.int64)
    labels = None if lab is None else np.zeros(len(p), np.int64)
    lib.centroid(_p(p, F32), len(p), _p(v, U8), _p(g, F32), _p(c, F32), len(g), ctypes.c_float(4), pos_num, _p(lab, I64),
                 _p(gt_inds, I64), _p(labels, I64))
    return gt_inds, labels


def run_atss(lib, boxes, level_len, flags, gt, gt_labels):
    b, g, v = _f(boxes), _f(gt), _u8(flags)
    lab = None if gt_labels is None else np.ascontiguousarray(gt_labels.numpy(), dtype=np.int64)
    lens = (ctypes.c_int * len(level_len))(*level_len)
    n = len(b)
    gt_inds, mo = np.zeros(n, np.int64), np.zeros(n, np.float32)
    labels = None if lab is None else np.zeros(n, np.int64)
    lib.atss(_p(b, F32), b.shape[1], n, len(level_len), lens, _p(v, U8), _p(g, F32), len(g), rc.TOPK, _p(lab, I64),
             _p(gt_inds, I64), _p(mo, F32), _p(labels, I64))
    return gt_inds, mo, labels


def test_table_and_input_condition(images):
    """The cases are what their table says, and every one meets the near-tie condition on its filtered inputs."""
    for k, ((h, w), counts, kept) in rc.IMAGES.items():
        im = images[k]
        assert im['counts'] == counts and [int(f.sum()) for f in torch.split(im['flags'], im['level_len'])] == counts, k
        assert len(im['boxes']) == kept, k
        assert rc.margins_ok(im), f'a near-tie in the filtered inputs of case {k}: replace it in assign_ragged_cases.IMAGES'
    assert len(images[None]['boxes']) == 0


@pytest.mark.parametrize('index', list(rc.IMAGES))
def test_masked_driver_matches_the_filtered_torch_statement(rows, images, index):
    im = images[index]
    flags = None if index == 0 else im['flags']       # the all-valid image also states the valid == NULL case
    for pos_num, typ in ac.CENTROID_MODES:
        cen = CentroidAssigner.gen_centroid(im['extremes'], len(im['boxes'])) if typ == 'centroid' else None
        for with_labels in (True, False):
            want_inds, want_labels = rc.centroid_statement(im, pos_num, typ, with_labels)
            got, labels = run_centroid(rows, im['pts'], flags, im['boxes'], cen, pos_num, im['labels'] if with_labels else None)
            assert (want_inds > 0).any() and np.array_equal(got, want_inds.numpy()), (pos_num, typ)
            assert (labels is None) == (not with_labels) and (labels is None or np.array_equal(labels, want_labels.numpy()))
            assert not got[~im['flags'].numpy()].any()
    props5 = torch.cat([im['props'], torch.rand(len(im['props']), 1, generator=torch.Generator().manual_seed(5))], 1)
    for boxes in (im['props'], props5):                # ld = 4 and ld = 5
        want_inds, want_mo, want_labels = rc.atss_statement(im)
        got, mo, labels = run_atss(rows, boxes, im['level_len'], flags, im['boxes'], im['labels'])
        assert (want_inds > 0).any() and np.array_equal(got, want_inds.numpy())
        assert np.array_equal(labels, want_labels.numpy())
        assert np.array_equal(mo, want_mo.numpy())      # the same bits on positives, -1e8 elsewhere and outside the image
    got, mo, labels = run_atss(rows, im['props'], im['level_len'], flags, im['boxes'], None)
    assert labels is None and np.array_equal(got, rc.atss_statement(im, with_labels=False)[0].numpy())


def test_a_tie_across_the_mask(rows):
    """`four_equal_k1`: with point (96, 96) masked out the gt takes the next of its four equidistant points in row order."""
    pts, _ = ac.grid()
    xy = {(int(x), int(y)): i for i, (x, y, s) in enumerate(pts.tolist()) if s == 8}
    name, gts, _, _ = ac.centroid_ties()[0]
    assert name == 'four_equal_k1'
    flags = torch.ones(len(pts), dtype=torch.bool)
    flags[xy[(96, 96)]] = False
    for pos_num, expect in ((1, [(104, 96)]), (3, [(104, 96), (96, 104), (104, 104)])):
        want = torch.zeros(len(pts), dtype=torch.long)
        want[[xy[p] for p in expect]] = 1
        got, _ = run_centroid(rows, pts, flags, gts, None, pos_num, None)
        assert np.array_equal(got, want.numpy()), pos_num
        ref = CentroidAssigner(scale=4, pos_num=pos_num, iou_type='center').assign(pts[flags], gts, None)
        assert torch.equal(rc.scatter(flags, ref.gt_inds, 0), want), pos_num


@pytest.mark.parametrize('D', [4, 12, 123])
@pytest.mark.parametrize('with_labels', [True, False])
def test_targets_rule(rows, images, D, with_labels):
    """lsn_assign_targets_batch's rule on a batch of three images (all valid, ragged, ragged without gts) against the
    statements of LSHead._dense_targets + the scatter."""
    batch = [images[0], images[12], images[None]]
    P, B, background = len(batch[0]['pts']), 3, 80
    g = torch.Generator().manual_seed(60 + D)
    tables = [torch.randn(len(im['boxes']), D, generator=g) for im in batch]
    labs = [torch.randint(0, 80, (len(im['boxes']),), generator=g) for im in batch]
    gt_inds = torch.stack([rc.seeded_gt_inds(70 + i, im['flags'], len(im['boxes'])) for i, im in enumerate(batch)])
    valid = torch.stack([im['flags'] for im in batch])
    off = np.cumsum([0] + [len(t) for t in tables]).astype(np.int32)
    table, lab = _f(torch.cat(tables)), np.ascontiguousarray(torch.cat(labs).numpy(), dtype=np.int64)
    gi, v = np.ascontiguousarray(gt_inds.numpy()), _u8(valid)
    out = [np.empty((B, P, D), np.float32), np.empty((B, P), np.int64), np.empty((B, P), np.float32),
           np.empty((B, P, 4), np.float32), np.empty((B,), np.int64)]
    rows.targets(_p(gi, I64), _p(v, U8), P, B, off.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _p(table, F32), D,
                 _p(lab, I64) if with_labels else None, ctypes.c_longlong(background), _p(out[0], F32), _p(out[1], I64),
                 _p(out[2], F32), _p(out[3], F32), _p(out[4], I64))
    assert np.array_equal(out[4], (gt_inds > 0).sum(1).numpy()) and out[4][0] > 0 and out[4][1] > 0 and out[4][2] == 0
    for b, im in enumerate(batch):
        want = rc.targets_statement(gt_inds[b], im['flags'], tables[b], labs[b] if with_labels else None, background)
        for got, w in zip(out[:4], want[:4]):
            assert np.array_equal(got[b], w.numpy()), (b, D)
        assert out[4][b] == int(want[4])


def _head():
    from lsnet_amd.models import build_head
    from lsnet_amd.utils import ConfigDict
    from tests import golden_util as gu
    import copy
    cfg, tr, te = gu.head_cfg('bbox')
    cfg = ConfigDict(copy.deepcopy(cfg))
    cfg.update(train_cfg=ConfigDict(tr), test_cfg=ConfigDict(te))
    return build_head(cfg)


def test_get_points_caches_the_mask_and_the_counts():
    head = _head()
    sizes = [(-(-800 // s), -(-800 // s)) for s in ac.STRIDES]
    metas = [dict(pad_shape=(800, 800, 3)), dict(pad_shape=(600, 700, 3))]
    points, flags, all_valid = head.get_points(sizes, metas, torch.device('cpu'))
    mask, counts = head.get_valid(sizes, metas, torch.device('cpu'))
    assert not all_valid and mask.dtype == torch.bool and tuple(mask.shape) == (2, sum(p.shape[0] for p in points))
    assert counts == [rc.IMAGES[0][1], rc.IMAGES[1][1]]
    for b in range(2):
        assert torch.equal(mask[b], torch.cat(flags[b])) and torch.equal(mask[b], rc.region_flags(*metas[b]['pad_shape'][:2])[0])
        assert counts[b] == [int(f.sum()) for f in flags[b]] and all(type(n) is int for n in counts[b])
    again = head.get_valid(sizes, metas, torch.device('cpu'))
    assert again[0] is mask and again[1] is counts                     # built once per geometry
    assert head.get_points(sizes, metas, torch.device('cpu'))[1] is flags


def test_atss_batch_refuses_a_level_short_of_topk():
    """A valid region of 200 x 300: the stride-128 level keeps 2 x 3 = 6 < 9 cells.  The batched call answers None, so the
    caller assigns image by image and torch.topk's error on the filtered level stays what the user sees."""
    im = rc.image(1)
    flags, counts = rc.region_flags(200, 300)
    assert counts[-1] == 6
    a = ATSSAssigner(topk=9)
    boxes = torch.stack([im['props'], im['props']])
    full = [im['level_len'], counts]
    assert a.assign_batch(boxes, im['level_len'], [im['boxes'], im['boxes']],
                          valid=torch.stack([torch.ones_like(flags), flags]), valid_counts=full) is None
    with pytest.raises(RuntimeError):
        a.assign(im['props'][flags], counts, im['boxes'])
    from lsnet_amd.ops.hip_backend import HipBackend
    with pytest.raises(NotImplementedError, match='6 valid boxes on level 4'):
        HipBackend().atss_assign_batch(boxes, im['level_len'], [im['boxes'], im['boxes']], 9,
                                       valid=torch.stack([torch.ones_like(flags), flags]), valid_counts=full)


def test_library_argument_checks_need_no_gpu():
    from lsnet_amd import _lib
    lib = _lib.load()
    off = (ctypes.c_int * 3)(0, 3, 3)
    assert lib.lsn_centroid_assign_masked_batch(None, 0, None, None, None, 2, off, ctypes.c_float(4), 1, None, None, None, None,
                                                None) == -1
    assert b'centroid assign' in lib.lsn_last_error()
    lens = (ctypes.c_int * 2)(100, 5)
    assert lib.lsn_atss_assign_masked_batch(None, 4, 105, 2, lens, None, None, 2, off, 9, None, None, None, None, None, None) == -1
    assert b'level 1 has 5 boxes' in lib.lsn_last_error()
    assert lib.lsn_assign_targets_batch(None, None, 5, 2, off, None, 0, None, 80, None, None, None, None, None, None) == -1
    assert b'assign targets' in lib.lsn_last_error()
    bad = (ctypes.c_int * 3)(1, 3, 3)
    assert lib.lsn_assign_targets_batch(None, None, 5, 2, bad, None, 4, None, 80, None, None, None, None, None, None) == -1
    assert b'gt_offset must start at 0' in lib.lsn_last_error()
