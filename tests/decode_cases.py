"""Inputs and torch references of the native-decode tests (tests/test_decode_host.py, tests/test_decode_gpu.py).

Head outputs come from gu.decode_inputs (candidate scores >= 1e-3 apart, so no decision hangs on the last bit of a sigmoid);
the reference is LSHead.get_bboxes on CPU tensors -- the torch statements, never the code under test.  The grids are small
enough for every case to take well under a second and chosen so that with nms_pre = 12 one level lies above the top-k
(9 x 13 and two more), one equals it (3 x 4) and one is a single point; img_shape = (70, 101) is smaller than the grids'
extent, so the clamps bite."""
import copy

import numpy as np
import torch

from tests import golden_util as gu

GRIDS = [(9, 13), (6, 8), (5, 7), (3, 4), (1, 1)]
BATCH, CLASSES, IMG, NMS_PRE, SEED = 3, 8, (70, 101), 12, 5
TASKS = ('bbox', 'segm', 'pose_bbox', 'pose_kbox')
CFG = dict(nms_pre=NMS_PRE, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_thr=0.6), max_per_img=100)

_heads = {}


def head(task, num_classes=CLASSES):
    """An LSHead of the task on the CPU (parameters unused: get_bboxes reads only the configuration)."""
    from lsnet_amd.models import build_head
    from lsnet_amd.utils import ConfigDict
    key = (task, num_classes)
    if key not in _heads:
        cfg, train_cfg, test_cfg = gu.head_cfg(task, 32, num_classes)
        cfg = ConfigDict(copy.deepcopy(cfg))
        cfg.update(train_cfg=ConfigDict(train_cfg), test_cfg=ConfigDict(test_cfg))
        _heads[key] = build_head(cfg).eval()
    return _heads[key]


def config(**kw):
    from lsnet_amd.utils import ConfigDict
    cfg = copy.deepcopy(CFG)
    nms = kw.pop('nms', None)
    cfg.update(kw)
    if nms:
        cfg['nms'].update(nms)
    return ConfigDict(cfg)


def inputs(task, seed=SEED, num_classes=CLASSES, batch=BATCH, grids=GRIDS):
    """(outs, min score gap): LSHead.forward's seven lists on the CPU, absent branches as lists of None."""
    h = head(task, num_classes)
    nv = h.num_vectors
    width = {'bbox': 20, 'segm': 4 * (nv + 1), 'pose': 4 * (nv + 1)}
    have = {'bbox': task in ('bbox', 'pose_bbox'), 'segm': task == 'segm', 'pose': task in ('pose_bbox', 'pose_kbox')}
    outs = [[torch.zeros(batch, num_classes, *g) for g in grids]]
    for b in ('bbox', 'segm', 'pose'):
        for _ in ('init', 'refine'):
            outs.append([torch.zeros(batch, width[b], *g) if have[b] else None for g in grids])
    return gu.decode_inputs(outs, seed, num_classes)


def metas(batch=BATCH, scale_factor=1.0, img=IMG):
    return [dict(img_shape=(img[0], img[1], 3), pad_shape=(img[0], img[1], 3), scale_factor=scale_factor) for _ in range(batch)]


def torch_path(task, outs, cfg, rescale=False, scale_factor=1.0, num_classes=CLASSES, img=IMG):
    """The torch statements on the CPU -> [(dets, vecs, labels)] as numpy arrays."""
    h = head(task, num_classes)
    with torch.no_grad():
        res = h.get_bboxes(*outs, metas(outs[0][0].shape[0], scale_factor, img), cfg=cfg, rescale=rescale)
    return [tuple(t.numpy() for t in r) for r in res]


def raw_candidates(task, outs, cfg, num_classes=CLASSES, img=IMG):
    """Candidates per image (point, class pairs above score_thr after the top-k), from the nms=False form."""
    h = head(task, num_classes)
    with torch.no_grad():
        res = h.get_bboxes(*outs, metas(outs[0][0].shape[0], img=img), cfg=cfg, nms=False)
    return [int((s[:, :-1] > cfg.score_thr).sum()) for _, _, s in res]


def dense_inputs(task, grids, num_classes, batch, cells_per_level, seed):
    """Head outputs with MANY candidates: per image and level, cells_per_level[l] random (class, y, x) cells (None: all of them)
    carry scores that are a random permutation of an evenly spaced grid over [0.06, 0.96] -- distinct, 0.9 / n apart -- the
    rest a background near -9; regression maps as gu.decode_inputs makes them.  -> (outs, smallest score gap)."""
    outs, _ = inputs(task, seed, num_classes, batch, grids)
    g = gu.gen(seed + 100)
    maps = [-9.0 - torch.rand(batch, num_classes, *gr, generator=g) for gr in grids]
    gap = 1.0
    for b in range(batch):
        picks = []
        for l, gr in enumerate(grids):
            n = num_classes * gr[0] * gr[1]
            k = n if cells_per_level[l] is None else cells_per_level[l]
            picks.append(torch.randperm(n, generator=g)[:k])
        total = sum(len(p) for p in picks)
        score = 0.06 + 0.9 * (torch.randperm(total, generator=g).double() + 0.5) / total
        logit = torch.log(score / (1 - score)).float()
        got = torch.sort(logit.sigmoid().double())[0]
        gap = min(gap, float((got[1:] - got[:-1]).min()))
        at = 0
        for l, p in enumerate(picks):
            maps[l][b].view(-1)[p] = logit[at:at + len(p)]
            at += len(p)
    outs[0] = maps
    return outs, gap


# The sizes at which the kernels change what a thread does (csrc/decode.hip): a level above 1024 points gives every thread of
# the select several rows; above 1024 candidates the greedy NMS walks several chunks; above 4096 the sort leaves its LDS tile.
BIG_IMG = (800, 1344)
_big = {}


def big_select_case():
    """100 x 168 and 6 x 8, C = 1, nms_pre = 1000 as shipped: 3000 candidate points on the large level, of which the top-k
    keeps 1000, and all 48 of the small one: 1048 candidates per image, two chunks of the NMS.  max_per_img = 2000 keeps
    every survivor, so the walk does not stop in the first chunk.  -> (outs, cfg, torch reference)."""
    if 'select' not in _big:
        grids = [(100, 168), (6, 8)]
        outs, gap = dense_inputs('bbox', grids, 1, 2, [3000, None], seed=21)
        cfg = config(nms_pre=1000, max_per_img=2000, nms=dict(iou_thr=0.1))      # (the boxes are small: 0.1 makes the NMS bite)
        assert gap > 1e-4 and grids[0][0] * grids[0][1] > 1024
        cands = raw_candidates('bbox', outs, cfg, 1, BIG_IMG)
        assert min(cands) > 1024 and min(raw_candidates('bbox', outs, config(nms_pre=-1), 1, BIG_IMG)) > min(cands)
        want = torch_path('bbox', outs, cfg, num_classes=1, img=BIG_IMG)
        # suppression happens, and the walk is not cut by max_per_img: it goes through the second chunk to the last candidate
        assert all(100 < len(w[0]) < cfg.max_per_img for w in want) and any(len(w[0]) < n for w, n in zip(want, cands))
        _big['select'] = (outs, cfg, want)
    return _big['select']


def big_sort_case():
    """The small grids with C = 40 and every (point, class) cell a candidate, nms_pre = -1: 213 x 40 = 8520 candidates in an
    image, above the sort's 4096-word tile (and below the cap of 16 384).  -> (outs, cfg, torch reference)."""
    if 'sort' not in _big:
        outs, gap = dense_inputs('bbox', GRIDS, 40, 2, [None] * len(GRIDS), seed=22)
        cfg = config(nms_pre=-1, max_per_img=2000)
        assert gap > 1e-4
        cands = raw_candidates('bbox', outs, cfg, 40)
        assert min(cands) > 4096 and max(cands) <= 16384
        want = torch_path('bbox', outs, cfg, num_classes=40)
        assert all(100 < len(w[0]) < n for w, n in zip(want, cands))
        _big['sort'] = (outs, cfg, want)
    return _big['sort']


_refs = {}


def reference(task):
    """The shared reference of a task at the standard shapes: (outs, dets at max_per_img = 100, dets at max_per_img = 10, dets
    at iou_thr = 0.1), with the conditions that make a passing case a non-empty one asserted on it.  (At iou_thr = 0.6 the
    small boxes of the two extreme-point tasks hardly overlap -- bbox loses 1 candidate of 106, pose_bbox none -- so the NMS
    condition is asserted on the 0.1 run, where every task loses some.)"""
    if task not in _refs:
        outs, gap = inputs(task)
        assert gap >= 0.02
        full = torch_path(task, outs, config())
        cut = torch_path(task, outs, config(max_per_img=10))
        tight = torch_path(task, outs, config(nms=dict(iou_thr=0.1)))
        cands, all_cands = raw_candidates(task, outs, config()), raw_candidates(task, outs, config(nms_pre=-1))
        assert any(a < b for a, b in zip(cands, all_cands)), 'the top-k cuts no candidate'
        assert any(len(a[0]) < n for a, n in zip(tight, cands)), 'the NMS suppresses nothing'
        assert all(len(a[0]) > 10 and len(c[0]) == 10 for a, c in zip(full, cut)), 'max_per_img = 10 does not cut every image'
        _refs[task] = (outs, full, cut, tight)
    return _refs[task]


def assert_same(got, want, what=''):
    """Labels, order and coordinates equal; scores within 1e-6 (two fp32 sigmoids of values <= 1, each a few ulp of 6e-8 off).
    Returns the largest score difference."""
    worst = 0.0
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        gd, gv, gl = (np.asarray(t) for t in g)
        wd, wv, wl = w
        assert gd.shape == wd.shape and gv.shape == wv.shape and gl.shape == wl.shape, (what, i, gd.shape, wd.shape, gv.shape, wv.shape)
        assert gd.dtype == wd.dtype and gv.dtype == wv.dtype and gl.dtype == wl.dtype, (what, i)
        assert np.array_equal(gl, wl), f'{what} image {i}: labels / order'
        assert np.array_equal(gd[:, :4], wd[:, :4]), f'{what} image {i}: boxes'
        assert np.array_equal(gv, wv), f'{what} image {i}: vectors'
        if len(gd):
            err = float(np.abs(gd[:, 4] - wd[:, 4]).max())
            assert err <= 1e-6, f'{what} image {i}: scores off by {err:.3e}'
            worst = max(worst, err)
    return worst
