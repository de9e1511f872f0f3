"""The staleness rules of the prepared-weight-image cache (lsnet_amd/ops/weight_images.py), one by one, on the host: CPU
tensors have version counters and storage pointers like device tensors, and the module's three doors to the library
(`_math_mode`, `_build_one`, `_rebuild_many`) are replaced by recorders -- no GPU, no library call."""
import gc

import pytest
import torch
import torch.nn as nn

from lsnet_amd.ops import weight_images as wi


class _Calls:
    def __init__(self):
        self.built, self.rebuilt, self.mode = [], [], 2

    def build_one(self, ent, w):
        if ent.image is None:       # (what the real one does for a new entry, minus the library's size)
            ent.image = torch.empty(8, dtype=torch.uint8)
            if ent.norm is not None and ent.key.kind == 0:
                ent.shift = torch.empty(w.shape[0])
        self.built.append(ent.key)

    def rebuild_many(self, items):
        assert all(ent.weight() is w for ent, w in items)
        self.rebuilt.append({ent.key for ent, _ in items})


@pytest.fixture
def calls(monkeypatch):
    c = _Calls()
    monkeypatch.setattr(wi, '_math_mode', lambda: c.mode)
    monkeypatch.setattr(wi, '_build_one', c.build_one)
    monkeypatch.setattr(wi, '_rebuild_many', c.rebuild_many)
    monkeypatch.setattr(wi, '_images', {})
    monkeypatch.setattr(wi, '_folded', {})
    return c


def _weight(trainable=False, co=8):
    return nn.Parameter(torch.randn(co, 4, 3, 3), requires_grad=trainable)


def _norm(co=8, trainable=False):
    bn = nn.BatchNorm2d(co).eval()
    bn.weight.requires_grad_(trainable), bn.bias.requires_grad_(trainable)
    return bn


def _entry(w, kind=0, stride=1, pad=0, dil=1, bn=None):
    (ent,) = [e for k, e in wi._images.items() if e.weight() is w and (k.kind, k.stride, k.pad, k.dil) == (kind, stride, pad, dil)
              and k.norm_id == (id(bn) if bn is not None else 0) and k.mode == wi._math_mode()]
    return ent


def _optimizer_step_elsewhere():
    """A real optimizer steps on ANOTHER parameter: only the global post-step hook can tell the cache."""
    p = nn.Parameter(torch.zeros(2))
    p.grad = torch.ones(2)
    torch.optim.SGD([p], lr=0.1).step()


def test_fresh_entry_is_not_stale_and_is_served_from_the_cache(calls):
    w = _weight(trainable=True)
    img = wi.weight_image(w, 0)
    assert not _entry(w).stale(w) and len(calls.built) == 1
    assert wi.weight_image(w, 0) is img
    assert len(calls.built) == 1 and calls.rebuilt == []
    assert wi.cached_kinds(w) == {0}


def test_in_place_write_rebuilds_every_stale_image_of_the_mode_in_one_call(calls):
    w, v, frozen = _weight(), _weight(), _weight()
    for t in (w, v, frozen):
        wi.weight_image(t, 0)
    wi.weight_image(w, 1, 2, 1, 1)
    calls.mode = 1
    wi.weight_image(w, 0)                     # the same tensor under another math mode: an entry of its own
    calls.mode = 2
    with torch.no_grad():
        w.add_(1.0), v.mul_(2.0)
    assert _entry(w).stale(w) and _entry(w, 1, 2, 1, 1).stale(w) and _entry(v).stale(v) and not _entry(frozen).stale(frozen)
    img = wi.weight_image(v, 0)
    mode2 = {k for k in wi._images if k.mode == 2}
    assert calls.rebuilt == [{k for k in mode2 if k.weight_id in (id(w), id(v))}] and len(calls.rebuilt[0]) == 3
    assert not _entry(w).stale(w) and not _entry(w, 1, 2, 1, 1).stale(w) and not _entry(v).stale(v)
    assert wi.weight_image(v, 0) is img and len(calls.rebuilt) == 1
    calls.mode = 1
    wi.weight_image(w, 0)                     # the other mode's image went stale with the same write: its own rebuild
    assert len(calls.rebuilt) == 2 and len(calls.rebuilt[1]) == 1


@pytest.mark.parametrize('tell', [_optimizer_step_elsewhere, wi.parameters_updated], ids=['optimizer_step', 'parameters_updated'])
def test_an_optimizer_step_stales_trainable_weights_only(calls, tell):
    frozen, trained, bn_frozen, bn_trained = _weight(False), _weight(True), _norm(), _norm(trainable=True)
    wi.weight_image(frozen, 0)
    wi.weight_image(trained, 0)
    wi.weight_image(frozen, 1, bn=bn_frozen)
    wi.weight_image(frozen, 1, bn=bn_trained)     # a frozen weight under a norm that trains: the image moves with gamma
    tell()
    assert not _entry(frozen).stale(frozen) and not _entry(frozen, 1, bn=bn_frozen).stale(frozen)
    assert _entry(trained).stale(trained) and _entry(frozen, 1, bn=bn_trained).stale(frozen)
    wi.weight_image(trained, 0)
    assert calls.rebuilt == [{_entry(trained).key, _entry(frozen, 1, bn=bn_trained).key}]


def test_replaced_storage_is_stale_though_the_version_stands(calls):
    w = _weight()
    wi.weight_image(w, 0)
    version = w._version
    w.data = torch.randn(8, 4, 3, 3)
    assert w._version == version and _entry(w).stale(w)


@pytest.mark.parametrize('what', ['weight', 'bias', 'running_mean', 'running_var', 'eps'])
def test_folded_norm_moves_the_image(calls, what):
    w, bn = _weight(), _norm()
    img, shift = wi.weight_image(w, 0, bn=bn)
    assert shift is not None and not _entry(w, bn=bn).stale(w)
    if what == 'eps':
        bn.eps = 2e-5
    else:
        with torch.no_grad():
            getattr(bn, what).add_(0.5)
    assert _entry(w, bn=bn).stale(w)
    again = wi.weight_image(w, 0, bn=bn)
    assert again[0] is img and again[1] is shift
    assert calls.rebuilt == [{_entry(w, bn=bn).key}] and not _entry(w, bn=bn).stale(w)


def test_an_entry_whose_norm_was_collected_is_skipped_not_rebuilt(calls):
    w, v, bn = _weight(), _weight(), _norm()
    wi.weight_image(w, 0, bn=bn)
    wi.weight_image(v, 0)
    orphan = _entry(w, bn=bn)
    del bn
    gc.collect()
    assert orphan.norm is not None and orphan.bn() is None and orphan.stale(w)
    with torch.no_grad():
        v.add_(1.0)
    wi.weight_image(v, 0)
    assert calls.rebuilt == [{_entry(v).key}]


def test_invalidate_stales_every_entry(calls):
    frozen, trained, bn = _weight(False), _weight(True), _norm()
    wi.weight_image(frozen, 0)
    wi.weight_image(frozen, 0, bn=bn)
    wi.weight_image(trained, 1, 1, 1, 1)
    wi.invalidate_weight_images()
    assert all(ent.stale(ent.weight()) for ent in wi._images.values()) and len(wi._images) == 3
    wi.weight_image(frozen, 0)
    assert calls.rebuilt == [set(wi._images)]
    assert not any(ent.stale(ent.weight()) for ent in wi._images.values())


def test_entries_go_with_their_weight(calls):
    w = _weight()
    wi.weight_image(w, 0)
    wi.weight_image(w, 2, 1, 1, 1)
    assert wi.cached_kinds(w) == {0, 2} and len(wi._images) == 2
    del w
    gc.collect()
    assert wi._images == {}
    assert wi.cached_kinds(_weight()) == set()


def test_geometry_and_norm_get_entries_of_their_own(calls):
    w, bn, other = _weight(), _norm(), _norm()
    asked = [(0, 1, 0, 1, None), (1, 1, 0, 1, None), (0, 2, 0, 1, None), (0, 1, 1, 1, None), (0, 1, 1, 2, None),
             (0, 1, 0, 1, bn), (0, 1, 0, 1, other)]
    images = [wi.weight_image(w, kind, s, p, d, bn=n) for kind, s, p, d, n in asked]
    assert len(wi._images) == len(asked) == len(calls.built)
    assert len({id(i[0] if isinstance(i, tuple) else i) for i in images}) == len(asked)
    assert wi.cached_kinds(w) == {0, 1}
    for (kind, s, p, d, n), img in zip(asked, images):      # each served again as it is, nothing built
        again = wi.weight_image(w, kind, s, p, d, bn=n)
        assert (again[0] is img[0] and again[1] is img[1]) if n is not None else again is img
    assert len(calls.built) == len(asked) and calls.rebuilt == []


def test_fold_bn_returns_the_same_objects_until_a_version_moves(calls):
    conv, bn = nn.Conv2d(4, 8, 3, bias=False), _norm()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 2.0), bn.bias.normal_(), bn.running_mean.normal_(), bn.running_var.uniform_(0.5, 2.0)
    w, shift = wi._fold_bn(conv, bn)
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    torch.testing.assert_close(w, conv.weight * scale.view(-1, 1, 1, 1))
    torch.testing.assert_close(shift, bn.bias - bn.running_mean * scale)
    again = wi._fold_bn(conv, bn)
    assert again[0] is w and again[1] is shift
    for t in (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var):
        with torch.no_grad():
            t.mul_(1.5)
        new = wi._fold_bn(conv, bn)
        assert new[0] is not w and new[1] is not shift
        w, shift = wi._fold_bn(conv, bn)
        assert w is new[0] and shift is new[1]
