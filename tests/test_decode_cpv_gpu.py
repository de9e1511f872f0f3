"""lsn_decode_cpv_batch behind LSCPVHead.get_bboxes on the device against the torch statements on the CPU, on the same bits
(tests/cpv_decode_cases.py: the grids, batch, classes, image and nms_pre of tests/decode_cases.py, corner maps of
gu.cpv_decode_inputs).  Labels, order and box coordinates np.array_equal, scores within 1e-6.  The reference asserts that the
top-k, the NMS and max_per_img = 10 cut, that the verification moves every candidate of the levels 1..4, that all four window
positions win an arg-max and that the cell clamp bites, so a passing case is not an empty one.  Every native case asserts
exactly one library call per get_bboxes."""
import numpy as np
import pytest
import torch

from lsnet_amd.models.dense_heads import ls_head
from tests import cpv_decode_cases as cc

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def to_device(outs, layout='nchw'):
    """nchw / nhwc: every map in that memory format.  slice: the two corner maps of a level are channel slices of ONE wider
    channels-last tensor whose other channels are NaN."""
    if layout == 'nchw':
        return [[t.to(DEV) for t in lv] for lv in outs]
    if layout == 'nhwc':
        return [[t.to(DEV).contiguous(memory_format=torch.channels_last) for t in lv] for lv in outs]
    dev = [[t.to(DEV) for t in lv] for lv in outs]
    for l, (score, off) in enumerate(zip(outs[3], outs[4])):
        B, _, H, W = score.shape
        wide = torch.full((B, 13, H, W), float('nan'), device=DEV).contiguous(memory_format=torch.channels_last)
        wide[:, 3:5], wide[:, 6:10] = score.to(DEV), off.to(DEV)
        dev[3][l], dev[4][l] = wide[:, 3:5], wide[:, 6:10]
    return dev


class Spy:
    """Counts the calls of HipBackend.decode_cpv_batch and keeps the last counts."""

    def __init__(self, monkeypatch):
        from lsnet_amd.ops.hip_backend import HipBackend
        self.calls, self._counts = 0, None
        inner = HipBackend.decode_cpv_batch

        def wrapped(backend, *a, **kw):
            out = inner(backend, *a, **kw)
            self.calls += 1
            self._counts = out[2]           # read when asked for: no synchronisation of the test's own inside get_bboxes
            return out
        monkeypatch.setattr(HipBackend, 'decode_cpv_batch', wrapped)

    @property
    def counts(self):
        return self._counts.cpu().tolist()


def device_path(outs, cfg, layout='nchw', rescale=False, scale_factor=1.0, as_numpy=True, img=cc.IMG):
    dev = to_device(outs, layout)
    with torch.no_grad():
        res = cc.head().get_bboxes(*dev, cc.metas(outs[0][0].shape[0], scale_factor, img), cfg=cfg, rescale=rescale)
    torch.cuda.synchronize()
    return [tuple(t.cpu().numpy() for t in r) for r in res] if as_numpy else res


@pytest.mark.parametrize('layout', ['nchw', 'nhwc', 'slice'])
def test_layouts(monkeypatch, layout):
    spy = Spy(monkeypatch)
    outs, full, cut, tight = cc.reference()
    cc.assert_same(device_path(outs, cc.config(), layout), full, f'cpv {layout}')
    assert spy.calls == 1 and spy.counts == [len(w[0]) for w in full]
    cc.assert_same(device_path(outs, cc.config(max_per_img=10), layout), cut, f'cpv {layout} max_per_img 10')
    cc.assert_same(device_path(outs, cc.config(nms=dict(iou_thr=0.1)), layout), tight, f'cpv {layout} iou 0.1')
    assert spy.calls == 3 and min(spy.counts) >= 0


def test_all_points_of_every_level(monkeypatch):
    spy = Spy(monkeypatch)
    outs = cc.reference()[0]
    cfg = cc.config(nms_pre=-1)
    cc.assert_same(device_path(outs, cfg), cc.torch_path(outs, cfg), 'cpv all points')
    assert spy.calls == 1


def test_scale_factors(monkeypatch):
    spy = Spy(monkeypatch)
    outs = cc.reference()[0]
    for sf in (1.5, np.array([1.25, 1.5, 1.75, 2.0], np.float32)):      # four distinct factors: every column's own divisor
        want = cc.torch_path(outs, cc.config(), rescale=True, scale_factor=sf)
        assert all(len(w[0]) for w in want)
        cc.assert_same(device_path(outs, cc.config(), rescale=True, scale_factor=sf), want, f'cpv scale {sf}')
    assert spy.calls == 2


def test_class_agnostic(monkeypatch):
    spy = Spy(monkeypatch)
    outs, full = cc.reference()[:2]
    cfg = cc.config(nms=dict(class_agnostic=True))
    want = cc.torch_path(outs, cfg)
    assert sum(len(w[0]) for w in want) < sum(len(w[0]) for w in full), 'class-agnostic NMS suppresses no more than per-class NMS'
    cc.assert_same(device_path(outs, cfg), want, 'cpv class-agnostic')
    assert spy.calls == 1


def test_images_without_candidates(monkeypatch):
    """Zero rows with the torch path's shapes and dtypes, for one image of a batch and for a whole batch."""
    spy = Spy(monkeypatch)
    outs = cc.reference()[0]
    one = [list(lv) for lv in outs]
    one[0] = [t.clone() for t in outs[0]]
    for t in one[0]:
        t[1] = -9.0
    want = cc.torch_path(one, cc.config())
    assert len(want[0][0]) and want[1][0].shape == (0, 5) and want[1][1].shape == (0,) and len(want[2][0])
    assert want[1][0].dtype == np.float32 and want[1][1].dtype == np.int64
    cc.assert_same(device_path(one, cc.config()), want, 'cpv image 1 empty')
    none = [list(lv) for lv in outs]
    none[0] = [torch.full_like(t, -9.0) for t in outs[0]]
    want = cc.torch_path(none, cc.config())
    assert all(w[0].shape == (0, 5) and w[1].shape == (0,) for w in want)
    cc.assert_same(device_path(none, cc.config()), want, 'cpv empty batch')
    assert spy.calls == 2 and spy.counts == [0, 0, 0]


def test_cand_cap_below_an_images_candidates(monkeypatch):
    """The image above the cap is decoded by the torch statements (on the device) and equals the torch path; the others are
    the native rows."""
    spy = Spy(monkeypatch)
    outs, full = cc.reference()[:2]
    cands = cc.raw_candidates(outs, cc.config())
    assert min(cands) < max(cands)
    monkeypatch.setattr(ls_head, 'DECODE_CAND_CAP', max(cands) - 1)
    cc.assert_same(device_path(outs, cc.config()), full, 'cpv cand_cap')
    assert spy.calls == 1
    assert [c < 0 for c in spy.counts] == [n > max(cands) - 1 for n in cands] and min(spy.counts) < 0 <= max(spy.counts)


def test_source_level_of_one_row_takes_the_torch_statements(monkeypatch):
    """Three levels whose second is 1 x 8: the stride-16 maps are no 2 x 2 source, the library call is not made."""
    spy = Spy(monkeypatch)
    outs, gap = cc.inputs(grids=[(9, 13), (1, 8), (5, 7)])
    assert gap > 1e-3
    want = cc.torch_path(outs, cc.config())
    assert all(len(w[0]) for w in want)
    cc.assert_same(device_path(outs, cc.config()), want, 'cpv 1 x 8 source')
    assert spy.calls == 0


def test_two_calls_give_the_same_bits(monkeypatch):
    spy = Spy(monkeypatch)
    outs = cc.reference()[0]
    a = device_path(outs, cc.config(), as_numpy=False)
    b = device_path(outs, cc.config(), as_numpy=False)
    assert spy.calls == 2
    for x, y in zip(a, b):
        assert len(x[0]) and all(torch.equal(s, t) for s, t in zip(x, y))


def test_switch_reproduces_the_torch_route(monkeypatch):
    """LSNET_NATIVE_DECODE=0 (the module flag it sets): the torch statements run on the device, the library call is not made."""
    spy = Spy(monkeypatch)
    monkeypatch.setattr(ls_head, 'NATIVE_DECODE', False)
    outs, full = cc.reference()[:2]
    cc.assert_same(device_path(outs, cc.config()), full, 'cpv switch off')
    assert spy.calls == 0
