"""lsn_decode_batch behind LSHead.get_bboxes on the device against the torch statements on the CPU, on the same bits
(tests/decode_cases.py: grids (9,13), (6,8), (5,7), (3,4), (1,1), B = 3, C = 8, img_shape (70, 101), nms_pre = 12).  Labels,
order and coordinates np.array_equal, scores within 1e-6.  The references assert that the top-k cuts candidates, that the NMS
suppresses and that max_per_img = 10 cuts every image, so a passing case is not an empty one.  The select keeps its keys in the
workspace at every level size, but three sizes change what a thread of the kernels does -- a level above 1024 points (several rows
per thread in the select), more than 1024 candidates (several chunks of the greedy NMS), more than 4096 (the sort leaves its LDS
tile): the last three cases cross each of them, at nms_pre = 1000 as shipped."""
import numpy as np
import pytest
import torch

from lsnet_amd.models.dense_heads import ls_head
from tests import decode_cases as dc

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def to_device(outs, layout='nchw'):
    def move(t):
        if t is None:
            return None
        if layout == 'nchw':
            return t.to(DEV)
        if layout == 'nhwc':
            return t.to(DEV).contiguous(memory_format=torch.channels_last)
        B, C, H, W = t.shape            # a channel slice of a wider channels-last tensor, as the head's concatenated outputs are
        wide = torch.full((B, C + 7, H, W), float('nan'), device=DEV).contiguous(memory_format=torch.channels_last)
        wide[:, 3:3 + C] = t.to(DEV)
        return wide[:, 3:3 + C]
    return [[move(t) for t in lv] for lv in outs]


class Spy:
    """Counts the calls of HipBackend.decode_batch and keeps the last counts."""

    def __init__(self, monkeypatch):
        from lsnet_amd.ops.hip_backend import HipBackend
        self.calls, self._counts = 0, None
        inner = HipBackend.decode_batch

        def wrapped(backend, *a, **kw):
            out = inner(backend, *a, **kw)
            self.calls += 1
            self._counts = out[3]           # read when asked for: no synchronisation of the test's own inside get_bboxes
            return out
        monkeypatch.setattr(HipBackend, 'decode_batch', wrapped)

    @property
    def counts(self):
        return self._counts.cpu().tolist()


def device_path(task, outs, cfg, layout='nchw', rescale=False, scale_factor=1.0, num_classes=dc.CLASSES, as_numpy=True, img=dc.IMG):
    h = dc.head(task, num_classes)
    dev = to_device(outs, layout)
    with torch.no_grad():
        res = h.get_bboxes(*dev, dc.metas(outs[0][0].shape[0], scale_factor, img), cfg=cfg, rescale=rescale)
    torch.cuda.synchronize()
    return [tuple(t.cpu().numpy() for t in r) for r in res] if as_numpy else res


@pytest.mark.parametrize('layout', ['nchw', 'nhwc', 'slice'])
@pytest.mark.parametrize('task', dc.TASKS)
def test_tasks_and_layouts(monkeypatch, task, layout):
    spy = Spy(monkeypatch)
    outs, full, cut, tight = dc.reference(task)
    dc.assert_same(device_path(task, outs, dc.config(), layout), full, f'{task} {layout}')
    dc.assert_same(device_path(task, outs, dc.config(max_per_img=10), layout), cut, f'{task} {layout} max_per_img 10')
    dc.assert_same(device_path(task, outs, dc.config(nms=dict(iou_thr=0.1)), layout), tight, f'{task} {layout} iou 0.1')
    assert spy.calls == 3 and min(spy.counts) >= 0


@pytest.mark.parametrize('task', dc.TASKS)
def test_scale_factors(monkeypatch, task):
    spy = Spy(monkeypatch)
    outs = dc.reference(task)[0]
    for sf in (1.5, np.array([1.25, 1.5, 1.75, 2.0], np.float32)):      # four distinct factors: every column's own divisor
        want = dc.torch_path(task, outs, dc.config(), rescale=True, scale_factor=sf)
        assert all(len(w[0]) for w in want)
        dc.assert_same(device_path(task, outs, dc.config(), rescale=True, scale_factor=sf), want, f'{task} scale {sf}')
    assert spy.calls == 2


@pytest.mark.parametrize('task', dc.TASKS)
def test_class_agnostic(monkeypatch, task):
    spy = Spy(monkeypatch)
    outs, full = dc.reference(task)[:2]
    cfg = dc.config(nms=dict(class_agnostic=True))
    want = dc.torch_path(task, outs, cfg)
    assert sum(len(w[0]) for w in want) < sum(len(w[0]) for w in full), 'class-agnostic NMS suppresses no more than per-class NMS'
    dc.assert_same(device_path(task, outs, cfg), want, f'{task} class-agnostic')
    assert spy.calls == 1


@pytest.mark.parametrize('task', ['bbox', 'pose_kbox'])
def test_images_without_candidates(monkeypatch, task):
    """Zero rows with the torch path's shapes and dtypes, for one image of a batch and for a whole batch."""
    spy = Spy(monkeypatch)
    outs = dc.reference(task)[0]
    one = [list(lv) for lv in outs]
    one[0] = [t.clone() for t in outs[0]]
    for t in one[0]:
        t[1] = -9.0
    want = dc.torch_path(task, one, dc.config())
    assert len(want[0][0]) and want[1][0].shape == (0, 5) and len(want[2][0])
    dc.assert_same(device_path(task, one, dc.config()), want, f'{task} image 1 empty')
    none = [list(lv) for lv in outs]
    none[0] = [torch.full_like(t, -9.0) for t in outs[0]]
    want = dc.torch_path(task, none, dc.config())
    assert all(w[0].shape == (0, 5) for w in want)
    dc.assert_same(device_path(task, none, dc.config()), want, f'{task} empty batch')
    assert spy.calls == 2 and spy.counts == [0, 0, 0]


@pytest.mark.parametrize('classes', [1, 80])
def test_class_counts(monkeypatch, classes):
    spy = Spy(monkeypatch)
    outs, gap = dc.inputs('bbox', seed=9, num_classes=classes)
    assert gap > 1e-3
    want = dc.torch_path('bbox', outs, dc.config(), num_classes=classes)
    assert all(len(w[0]) for w in want)
    dc.assert_same(device_path('bbox', outs, dc.config(), num_classes=classes), want, f'C={classes}')
    assert spy.calls == 1


def test_nan_logit_on_a_level_the_topk_cuts(monkeypatch):
    """A NaN ranks largest in the top-k (it takes one of the 12 places of level 0) and is no candidate."""
    spy = Spy(monkeypatch)
    outs, full = dc.reference('bbox')[:2]
    bad = [list(lv) for lv in outs]
    bad[0] = [t.clone() for t in outs[0]]
    score = bad[0][0][0].sigmoid().max(0)[0]
    assert int((score > 0.05).sum()) > dc.NMS_PRE           # more candidate points than places: the NaN pushes one out
    y, x = np.unravel_index(int(score.argmin()), score.shape)
    bad[0][0][0, 2, y, x] = float('nan')
    want = dc.torch_path('bbox', bad, dc.config())
    assert len(want[0][0]) == len(full[0][0]) - 1 and not np.isnan(want[0][0]).any()
    dc.assert_same(device_path('bbox', bad, dc.config()), want, 'NaN logit')
    assert spy.calls == 1


def test_cand_cap_below_an_images_candidates(monkeypatch):
    """The image above the cap is decoded by the torch statements (on the device) and equals the torch path; the others are
    the native rows."""
    spy = Spy(monkeypatch)
    outs, full = dc.reference('bbox')[:2]
    cands = dc.raw_candidates('bbox', outs, dc.config())
    assert min(cands) < max(cands)
    monkeypatch.setattr(ls_head, 'DECODE_CAND_CAP', max(cands) - 1)
    dc.assert_same(device_path('bbox', outs, dc.config()), full, 'cand_cap')
    assert spy.calls == 1
    assert [c < 0 for c in spy.counts] == [n > max(cands) - 1 for n in cands] and min(spy.counts) < 0 <= max(spy.counts)


def numpy_decode(raw, level_len, nms_pre, score_thr, iou_thr, class_agnostic, max_per_img, with_rows=False):
    """Steps 1 and 4-6 restated: raw = (boxes (n, 4), vecs, scores (n, C + 1)) of ALL points in (level, row) order.  Top-k per
    level by descending key, equal keys by ascending row; candidates ordered by descending score, equal scores by ascending
    (level, row, class); greedy NMS in separately rounded fp32 (numpy float32 arrays round every elementwise operation).
    with_rows: also the kept candidates' rows in the concatenation of the levels."""
    boxes, vecs, scores = (np.asarray(t, np.float32) for t in raw)
    scores = scores[:, :-1]
    rows, start = [], 0
    for n in level_len:
        key = scores[start:start + n].max(1)
        order = np.argsort(-key, kind='stable')             # stable: equal keys keep ascending rows
        rows += sorted(start + order[:nms_pre if 0 < nms_pre < n else n])
        start += n
    cand = [(-scores[r, c], r, c) for r in rows for c in range(scores.shape[1]) if scores[r, c] > np.float32(score_thr)]
    cand.sort()
    f = np.float32
    maxc = max(boxes[r].max() for _, r, _ in cand)
    kept, out = np.zeros((max_per_img, 4), f), []
    for _, r, c in cand:
        off = f(0) if class_agnostic else f(c) * (maxc + f(1))
        b = boxes[r] + off
        k = kept[:len(out)]
        w = np.maximum(f(0), np.minimum(k[:, 2], b[2]) - np.maximum(k[:, 0], b[0]))
        h = np.maximum(f(0), np.minimum(k[:, 3], b[3]) - np.maximum(k[:, 1], b[1]))
        inter = w * h
        union = ((k[:, 2] - k[:, 0]) * (k[:, 3] - k[:, 1]) + (b[2] - b[0]) * (b[3] - b[1])) - inter
        with np.errstate(invalid='ignore', divide='ignore'):        # 0 / 0 of two empty boxes: NaN, not above anything
            if (inter / union > f(iou_thr)).any():
                continue
        assert inter.dtype == np.float32 and union.dtype == np.float32
        kept[len(out)] = b
        out.append((r, c))
        if len(out) == max_per_img:
            break
    rr, cc = [r for r, _ in out], [c for _, c in out]
    dets = np.concatenate([boxes[rr], scores[rr, cc][:, None]], 1)
    res = (dets, vecs[rr], np.asarray(cc, np.int64))
    return res + (np.asarray(rr),) if with_rows else res


@pytest.mark.parametrize('class_agnostic', [False, True], ids=['per_class', 'agnostic'])
@pytest.mark.parametrize('nms_pre', [dc.NMS_PRE, -1])
def test_tie_rule(monkeypatch, nms_pre, class_agnostic):
    """Logits drawn from four values and regression maps from two, so that equal scores and identical boxes abound: the
    result follows step 4's total order -- the library's own rule, which the reference leaves to an unstable sort."""
    spy = Spy(monkeypatch)
    g = torch.Generator().manual_seed(3)
    outs = dc.inputs('bbox')[0]
    values = torch.tensor([-9.0, -0.5, 0.75, 2.0])
    outs[0] = [values[torch.randint(0, 4, t.shape, generator=g)] for t in outs[0]]
    outs[2] = [torch.tensor([0.5, 1.5])[torch.randint(0, 2, t.shape, generator=g)] for t in outs[2]]
    cfg = dc.config(nms_pre=nms_pre, max_per_img=40, nms=dict(class_agnostic=class_agnostic))
    h = dc.head('bbox')
    with torch.no_grad():
        raw = h.get_bboxes(*outs, dc.metas(), cfg=dc.config(nms_pre=-1), nms=False)
    got = device_path('bbox', outs, cfg)
    level_len = [a * b for a, b in dc.GRIDS]
    want = [numpy_decode([t.numpy() for t in r], level_len, nms_pre, cfg.score_thr, cfg.nms['iou_thr'], class_agnostic, 40)
            for r in raw]
    for w in want:
        assert len(w[0]) == 40 and len(np.unique(w[0][:, 4])) <= 3          # three scores above the threshold: ties everywhere
    dc.assert_same(got, want, 'ties')
    assert spy.calls == 1


@pytest.mark.parametrize('layout', ['nchw', 'slice'])
def test_level_above_1024_points_and_two_nms_chunks(monkeypatch, layout):
    """100 x 168 under nms_pre = 1000: every thread of the select owns 17 rows; 1048 candidates: the NMS walks two chunks."""
    spy = Spy(monkeypatch)
    outs, cfg, want = dc.big_select_case()
    dc.assert_same(device_path('bbox', outs, cfg, layout, num_classes=1, img=dc.BIG_IMG), want, 'large level')
    assert spy.calls == 1 and spy.counts == [len(w[0]) for w in want]


def test_more_than_4096_candidates(monkeypatch):
    """8520 candidates in an image: the sort runs 16 384 words through four LDS tiles and the wide strides of the workspace."""
    spy = Spy(monkeypatch)
    outs, cfg, want = dc.big_sort_case()
    dc.assert_same(device_path('bbox', outs, cfg, num_classes=40), want, 'many candidates')
    assert spy.calls == 1 and spy.counts == [2000, 2000]


@pytest.mark.parametrize('classes', [1, 3])
def test_tied_keys_at_the_cut_of_a_large_level(monkeypatch, classes):
    """Four-valued logits on 100 x 168, nms_pre = 1000: thousands of points share the largest key (a quarter of them at C = 1,
    over half at C = 3, where a point's classes tie as well) and the cut falls among them -- the lowest 1000 tied rows win, ranked inside and across the threads' 17-row chunks.
    max_per_img = 2000 and iou_thr = 0.1 let the walk reach the last candidate, so the rows at the cut are in the result:
    the reference asserts that its highest kept row of the level lies beyond the 900th tied row and that nms_pre = 999 gives
    another result.  Reference: numpy_decode (torch.topk does not promise the lower row among equals)."""
    spy = Spy(monkeypatch)
    g = torch.Generator().manual_seed(4)
    grids = [(100, 168), (6, 8)]
    level_len = [a * b for a, b in grids]
    outs = dc.inputs('bbox', 23, classes, 2, grids)[0]
    # (at C = 3 only the largest value passes score_thr: some 1300 candidates, so that max_per_img does not end the walk early)
    values = torch.tensor([-9.0, -0.5, 0.75, 2.0] if classes == 1 else [-9.0, -8.0, -7.0, 2.0])
    outs[0] = [values[torch.randint(0, 4, t.shape, generator=g)] for t in outs[0]]
    agnostic = False
    cfg = dc.config(nms_pre=1000, max_per_img=2000, nms=dict(iou_thr=0.1, class_agnostic=agnostic))
    h = dc.head('bbox', classes)
    with torch.no_grad():
        raw = h.get_bboxes(*outs, dc.metas(2, img=dc.BIG_IMG), cfg=dc.config(nms_pre=-1), nms=False)
    raw = [[t.numpy() for t in r] for r in raw]
    want = []
    for b, r in enumerate(raw):
        full = numpy_decode(r, level_len, 1000, cfg.score_thr, 0.1, agnostic, 2000, with_rows=True)
        tied = np.flatnonzero((outs[0][0][b].reshape(classes, -1) == 2.0).any(0).numpy())       # rows with the largest key
        assert len(tied) > 1000
        top = full[3][full[3] < level_len[0]].max()
        assert tied[900] < top <= tied[999], 'the kept rows do not reach the cut'
        assert len(full[0]) < 2000, 'max_per_img stops the walk before the last candidate'
        less = numpy_decode(r, level_len, 999, cfg.score_thr, 0.1, agnostic, 2000)
        assert len(less[0]) != len(full[0]) or not np.array_equal(less[0], full[0]), 'one place less changes nothing'
        want.append(full[:3])
    dc.assert_same(device_path('bbox', outs, cfg, num_classes=classes, img=dc.BIG_IMG), want, 'ties at the cut')
    assert spy.calls == 1 and spy.counts == [len(w[0]) for w in want]


def test_two_calls_give_the_same_bits(monkeypatch):
    spy = Spy(monkeypatch)
    outs = dc.reference('segm')[0]
    a = device_path('segm', outs, dc.config(), as_numpy=False)
    b = device_path('segm', outs, dc.config(), as_numpy=False)
    assert spy.calls == 2
    for x, y in zip(a, b):
        assert len(x[0]) and all(torch.equal(s, t) for s, t in zip(x, y))


def test_switch_reproduces_the_torch_route(monkeypatch):
    """LSNET_NATIVE_DECODE=0 (the module flag it sets): the torch statements run on the device, the library call is not made."""
    spy = Spy(monkeypatch)
    monkeypatch.setattr(ls_head, 'NATIVE_DECODE', False)
    outs, full = dc.reference('pose_bbox')[:2]
    dc.assert_same(device_path('pose_bbox', outs, dc.config()), full, 'switch off')
    assert spy.calls == 0
