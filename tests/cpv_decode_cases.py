"""Inputs and torch reference of the corner-verified decode tests (tests/test_decode_cpv_host.py, tests/test_decode_cpv_gpu.py).

Head outputs come from gu.cpv_decode_inputs at the shapes of tests/decode_cases.py: candidate scores and corner heat-map logits
lie far enough apart that no decision hangs on the last bit of a sigmoid.  The reference is LSCPVHead.get_bboxes on CPU tensors
-- the torch statements, never the code under test.  `reference` asserts on it what makes a passing case a non-empty one: the
top-k, max_per_img and the NMS all cut, every candidate of the levels 1..4 is moved by its verification, every position of the
2x2 window wins an arg-max somewhere, and the clamp of the cell index to the pooled map bites in x and in y."""
import copy

import numpy as np
import torch

from tests import decode_cases as dc
from tests import golden_util as gu

GRIDS, BATCH, CLASSES, IMG, NMS_PRE, SEED = dc.GRIDS, dc.BATCH, dc.CLASSES, dc.IMG, dc.NMS_PRE, dc.SEED
config, metas = dc.config, dc.metas

_heads = {}


def head():
    """An LSCPVHead on the CPU (parameters unused: get_bboxes reads only the configuration)."""
    from lsnet_amd.models import build_head
    from lsnet_amd.utils import ConfigDict
    if 'cpv' not in _heads:
        cfg, train_cfg, test_cfg = gu.cpv_head_cfg(32, CLASSES)
        cfg = ConfigDict(copy.deepcopy(cfg))
        cfg.update(train_cfg=ConfigDict(train_cfg), test_cfg=ConfigDict(test_cfg))
        _heads['cpv'] = build_head(cfg).eval()
    return _heads['cpv']


def inputs(seed=SEED, batch=BATCH, grids=GRIDS):
    """(outs, min score gap): LSCPVHead.forward's six lists (cls, bbox_init, bbox_refine, hm_score, hm_offset, sem) on the CPU."""
    widths = (CLASSES, 20, 20, 2, 4, CLASSES)
    outs = [[torch.zeros(batch, w, *g) for g in grids] for w in widths]
    return gu.cpv_decode_inputs(outs, seed, CLASSES)


def torch_path(outs, cfg, rescale=False, scale_factor=1.0, img=IMG):
    """The torch statements on the CPU -> [(dets, labels)] as numpy arrays."""
    with torch.no_grad():
        res = head().get_bboxes(*outs, metas(outs[0][0].shape[0], scale_factor, img), cfg=cfg, rescale=rescale)
    return [tuple(t.numpy() for t in r) for r in res]


def raw(outs, cfg, img=IMG):
    """[(boxes (n, 4), scores (n, C + 1))] of the selected points in (level, selection) order: the nms=False form."""
    with torch.no_grad():
        res = head().get_bboxes(*outs, metas(outs[0][0].shape[0], img=img), cfg=cfg, nms=False)
    return [(b.numpy(), s.numpy()) for b, s in res]


def raw_candidates(outs, cfg, img=IMG):
    return [int((s[:, :-1] > cfg.score_thr).sum()) for _, s in raw(outs, cfg, img)]


def heat_gap(outs, src):
    """Smallest difference between two sigmoid values of one image and channel of corner heat-map `src`."""
    sig = torch.sort(outs[3][src].double().sigmoid().flatten(2), dim=2)[0]
    return float((sig[..., 1:] - sig[..., :-1]).min())


def verification_facts(outs, cfg):
    """What the verification does to the candidates of the reference, restated from the unverified boxes (LSHead's
    statements on the same maps select the same rows): per level the candidates and how many of them moved, the window positions
    (0..3, row-major) that won an arg-max, and how often coordinate / stride exceeded the pooled map in x and in y."""
    B = outs[0][0].shape[0]
    with torch.no_grad():
        plain = dc.head('bbox', CLASSES).get_bboxes(outs[0], outs[1], outs[2], *[[None] * len(GRIDS)] * 4, metas(B), cfg=cfg,
                                                    nms=False)
    level_len = [min(cfg.nms_pre, h * w) if cfg.nms_pre > 0 else h * w for h, w in GRIDS]
    verify = head()._verify_sources(len(GRIDS))
    strides = head().point_strides
    cands, moved, wins, bite_x, bite_y = [0] * len(GRIDS), [0] * len(GRIDS), set(), 0, 0
    for b, ((boxes, scores), (pb, _, ps)) in enumerate(zip(raw(outs, cfg), plain)):
        assert np.array_equal(scores, ps.numpy())
        pb, start = pb.numpy(), 0
        for l, n in enumerate(level_len):
            rows = np.flatnonzero((scores[start:start + n, :-1] > cfg.score_thr).any(1)) + start
            cands[l] += len(rows)
            moved[l] += int((boxes[rows] != pb[rows]).any(1).sum())
            if verify[l] >= 0:
                s, heat = np.float32(strides[verify[l]]), outs[3][verify[l]][b].sigmoid().numpy()
                Hs, Ws = heat.shape[-2:]
                for r in rows:
                    for k in (0, 1):
                        fx, fy = pb[r, 2 * k] / s, pb[r, 2 * k + 1] / s
                        bite_x, bite_y = bite_x + (fx > Ws - 2), bite_y + (fy > Hs - 2)
                        cx, cy = int(np.floor(np.clip(fx, 0, Ws - 2))), int(np.floor(np.clip(fy, 0, Hs - 2)))
                        wins.add(int(np.argmax(heat[k, cy:cy + 2, cx:cx + 2].reshape(-1))))
            start += n
    return cands, moved, wins, int(bite_x), int(bite_y)


_ref = {}


def reference():
    """(outs, dets at max_per_img = 100, at max_per_img = 10, at iou_thr = 0.1), the conditions above asserted."""
    if not _ref:
        outs, gap = inputs()
        assert gap >= 0.019
        assert heat_gap(outs, 0) > 1e-3 and heat_gap(outs, 1) > 1e-3
        full = torch_path(outs, config())
        cut = torch_path(outs, config(max_per_img=10))
        tight = torch_path(outs, config(nms=dict(iou_thr=0.1)))
        cands, all_cands = raw_candidates(outs, config()), raw_candidates(outs, config(nms_pre=-1))
        assert any(a < b for a, b in zip(cands, all_cands)), 'the top-k cuts no candidate'
        assert any(len(a[0]) < n for a, n in zip(tight, cands)), 'the NMS suppresses nothing'
        assert all(len(a[0]) > 10 and len(c[0]) == 10 for a, c in zip(full, cut)), 'max_per_img = 10 does not cut every image'
        per_level, moved, wins, bite_x, bite_y = verification_facts(outs, config())
        assert moved[0] == 0 and all(n > 0 and m == n for n, m in zip(per_level[1:], moved[1:])), (per_level, moved)
        assert wins == {0, 1, 2, 3}, wins
        assert bite_x > 0 and bite_y > 0, (bite_x, bite_y)
        _ref['ref'] = (outs, full, cut, tight)
    return _ref['ref']


def assert_same(got, want, what=''):
    """Labels, order and coordinates equal; scores within 1e-6 (decode_cases.assert_same, without vectors).  Returns the
    largest score difference."""
    worst = 0.0
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        gd, gl = (np.asarray(t) for t in g)
        wd, wl = w
        assert gd.shape == wd.shape and gl.shape == wl.shape, (what, i, gd.shape, wd.shape, gl.shape, wl.shape)
        assert gd.dtype == wd.dtype and gl.dtype == wl.dtype, (what, i)
        assert np.array_equal(gl, wl), f'{what} image {i}: labels / order'
        assert np.array_equal(gd[:, :4], wd[:, :4]), f'{what} image {i}: boxes'
        if len(gd):
            err = float(np.abs(gd[:, 4] - wd[:, 4]).max())
            assert err <= 1e-6, f'{what} image {i}: scores off by {err:.3e}'
            worst = max(worst, err)
    return worst
