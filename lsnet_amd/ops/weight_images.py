"""The prepared weight images of the dense convolutions (ops/conv.py) and of the groups = 1 deformable layers
(ops/hip_backend.py): one image per (weight tensor OBJECT, pass, geometry, math mode, folded BatchNorm), rebuilt when the
weight moved on.  "Moved on" is inferred from the tensor's version counter and storage pointer, from the folded norm's
tensors and -- for trainable weights -- from the optimizer epoch that the global optimizer post-step hook advances;
whoever writes parameters behind all of these calls `invalidate_weight_images`.  The library is reached through
`_math_mode`, `_build_one` and `_rebuild_many` alone: tests/test_weight_images_host.py swaps them for recorders."""
import ctypes
import os
import weakref
from collections import namedtuple

import torch
from torch.optim.optimizer import register_optimizer_step_post_hook

from .. import _lib
from .._lib import stream
from .streams import side_stream

# LSNET_SIDE_STREAM_IMAGES=0: the images are rebuilt on the stream that asks for them (A/B switch)
SIDE_STREAM_IMAGES = os.environ.get('LSNET_SIDE_STREAM_IMAGES', '1') != '0'


class _State:
    epoch = 0            # advanced by every optimizer step (and by invalidate_weight_images)
    step_done = {}       # device index -> event recorded right behind the last optimizer step (on the stream that ran it)


# kind 0: forward, 1: backward data, 2: the deformable backward GEMM; mode: the library's math mode; norm_id: id(bn) or 0
ImageKey = namedtuple('ImageKey', 'weight_id kind stride pad dil mode norm_id')
_Folded = namedtuple('_Folded', 'weight norm versions folded shift')     # (weight, norm: weakrefs)
_images = {}             # ImageKey -> _Image
_folded = {}             # (id(conv.weight), id(bn)) -> _Folded


def _norm_versions(bn):
    return (bn.weight._version, bn.bias._version, bn.running_mean._version, bn.running_var._version,
            bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(), float(bn.eps))


class _Image:
    __slots__ = ('key', 'weight', 'version', 'storage', 'image', 'epoch', 'norm', 'shift', 'norm_versions')

    def __init__(self, key, w, bn):
        self.key, self.image, self.shift, self.norm_versions = key, None, None, None     # (image, shift: _build_one allocates them)
        self.weight = weakref.ref(w, lambda _, k=key: _images.pop(k, None))
        self.norm = weakref.ref(bn) if bn is not None else None
        self.mark_fresh(w)

    def bn(self):
        return self.norm() if self.norm is not None else None

    def is_for(self, w, bn):
        return self.weight() is w and (bn is None or self.bn() is bn)

    def moved(self, w):
        """Written, or given another storage, since the image was built -- whatever the optimizer epoch says."""
        return self.version != w._version or self.storage != w.data_ptr() or \
            (self.norm is not None and (self.bn() is None or self.norm_versions != _norm_versions(self.bn())))

    def stale(self, w):
        bn = self.bn()
        trainable = w.requires_grad or (bn is not None and (bn.weight.requires_grad or bn.bias.requires_grad))
        return self.moved(w) or (trainable and self.epoch != _State.epoch)

    def mark_fresh(self, w):
        self.version, self.storage, self.epoch = w._version, w.data_ptr(), _State.epoch
        if self.bn() is not None:
            self.norm_versions = _norm_versions(self.bn())

    def fill(self, it, w):
        """The library's job record (lsn_conv_wprep) of this image."""
        Co, C, kh, kw = w.shape
        k, bn = self.key, self.bn()
        it.kind, it.w, it.prepared = k.kind, w.data_ptr(), self.image.data_ptr()
        it.C, it.Co, it.kh, it.kw, it.stride, it.pad, it.dil = C, Co, kh, kw, k.stride, k.pad, k.dil
        if bn is not None:   # a BatchNorm folded into the image (lsn_conv_wprep); the shift belongs to the forward image
            it.bn_gamma, it.bn_var, it.bn_beta, it.bn_mean = bn.weight.data_ptr(), bn.running_var.data_ptr(), \
                bn.bias.data_ptr(), bn.running_mean.data_ptr()
            it.shift_out, it.bn_eps = (self.shift.data_ptr() if self.shift is not None else None), float(bn.eps)


def parameters_updated(*_):
    """Every image of a trainable weight is stale now.  The global optimizer post-step hook (the tensors' version counters
    are not enough: torch's FUSED optimizers update parameters without bumping them), and what optimizers that do not derive
    from torch.optim.Optimizer call themselves (runner/fused_sgd.py writes the parameters from its own kernel)."""
    _State.epoch += 1
    if SIDE_STREAM_IMAGES and torch.cuda.is_available() and torch.cuda.is_initialized() \
            and not torch.cuda.is_current_stream_capturing():
        dev = torch.cuda.current_device()
        ev = _State.step_done.get(dev)
        if ev is None:
            ev = _State.step_done[dev] = torch.cuda.Event()
        ev.record()


register_optimizer_step_post_hook(parameters_updated)     # (once per process: a module body runs once)


def invalidate_weight_images():
    """Mark EVERY cached image stale (frozen weights included).  Staleness is otherwise inferred from the tensors' version counters,
    their storage pointers and the global optimizer post-step hook -- in-place updates through `p.data` (checkpoint loading, the
    parameter broadcast of DataParallelModel, EMA / weight-surgery hooks, optimizers that do not derive from torch.optim.Optimizer)
    are invisible to all three: whoever writes parameters that way calls this.  GraphedForwardBackward also calls it right before
    a capture, so that the image-rebuild launches are ALWAYS recorded into the graph (captured with fresh images, every replay
    would run forward and data gradient on the capture-time weights while the optimizer keeps moving them)."""
    _State.epoch += 1
    _State.step_done.clear()    # (the writes this call stands for came after the optimizer step: no rebuild behind its event)
    for ent in _images.values():
        ent.version = -1


def cached_kinds(w):
    """The image kinds currently held for the tensor object `w` (tests)."""
    return {key.kind for key, ent in _images.items() if ent.weight() is w}


def _math_mode():
    return _lib.load().lsn_get_math_mode()


def _build_one(ent, w):
    """Build ONE image now, on the asking stream (lsn_conv2d_prepare_weights_item); a new entry gets its buffers first."""
    lib = _lib.load()
    if ent.image is None:
        Co, C, kh, kw = w.shape
        k = ent.key
        nbytes = lib.lsn_conv2d_prepared_bytes(k.kind, C, Co, kh, kw, k.stride, k.pad, k.dil)
        if nbytes < 0:
            _lib.check(-2)
        ent.image = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
        if ent.norm is not None and k.kind == 0:
            ent.shift = torch.empty(Co, device=w.device, dtype=torch.float32)
    it = _lib.ConvWprep()
    ent.fill(it, w)
    _lib.check(lib.lsn_conv2d_prepare_weights_item(ctypes.byref(it), stream()))


def _rebuild_many(items):
    """Rebuild the images of `items` [(entry, weight)] in one launch (lsn_conv2d_prepare_weights_multi)."""
    if torch.cuda.is_current_stream_capturing():
        # the multi-tensor launch uploads its job table when the set of stale images changed (a synchronous copy: not
        # allowed while a hipGraph is being captured): one launch per image instead, recorded into the graph
        for ent, w in items:
            _build_one(ent, w)
        return
    lib = _lib.load()
    arr = (_lib.ConvWprep * len(items))()
    for it, (ent, w) in zip(arr, items):
        ent.fill(it, w)
    dev = items[0][1].device.index
    ev = _State.step_done.get(dev) if SIDE_STREAM_IMAGES and len(items) > 1 else None
    # Behind the event only what the event is known to cover: every image here must be stale for ONE reason, the optimizer
    # epoch -- same tensor version and storage as when it was built, so that no torch operation has written the weight since
    # (any in-place write bumps the version) and the writer was the library's own optimizer kernel (runner/fused_sgd.py calls
    # parameters_updated() right behind it).  torch's optimizers bump the versions: their steps rebuild in stream order.
    if ev is None or not all(w.device.index == dev and not ent.moved(w) for ent, w in items):
        _lib.check(lib.lsn_conv2d_prepare_weights_multi(len(items), arr, stream()))
        return
    # The rebuild (one bandwidth-bound launch, ~0.2 ms for LSNet R-50) needs the optimizer step and nothing later: it runs on
    # a second stream behind the event recorded there, beside whatever the asking stream has queued since -- the frozen stem
    # and first stage of the next forward, whose images never change -- and the asking stream waits for it here.
    main = torch.cuda.current_stream(dev)
    side = side_stream(torch.device('cuda', dev))       # (ONE per process and device: ops/streams.py says why)
    side.wait_event(ev)
    with torch.cuda.stream(side):
        _lib.check(lib.lsn_conv2d_prepare_weights_multi(len(items), arr, stream()))
    main.wait_stream(side)


def _refresh_stale(mode):
    """Rebuild EVERY cached image of this math mode whose weight (or folded BatchNorm) has moved on -- all trainable
    convolutions after an optimizer step -- together: called when the first stale image of a step is asked for.  (An entry
    whose norm has been collected cannot be rebuilt; it goes with its weight.)"""
    items = [(ent, ent.weight()) for key, ent in _images.items() if key.mode == mode and (ent.norm is None or ent.bn() is not None)]
    items = [(ent, w) for ent, w in items if w is not None and ent.stale(w)]
    if items:
        _rebuild_many(items)
        for ent, w in items:
            ent.mark_fresh(w)


def weight_image(w, kind, stride=1, pad=0, dil=1, bn=None):
    """The prepared image (lsn_conv2d_prepare_weights) of a channels-last (Co, C, kh, kw) weight for the forward (kind 0) or
    backward-data (kind 1) pass, or a deformable layer's backward GEMM (kind 2).  Cached per tensor OBJECT; stale when the
    tensor's version counter or storage moved, or -- for a trainable weight -- when any optimizer has stepped since.  The stale
    images of all parameters are rebuilt together, once per optimizer step, when the first of them is needed; a temporary (padded
    view, test tensor) gets a fresh one and drops it when it dies.
    bn: an eval-mode BatchNorm2d folded into the image (every weight of forward output channel co scaled by gamma / sqrt(var + eps)).
    kind 0 returns (image, shift) -- the shift goes into the convolution's bias slot; kind 1 the image of the scaled weight."""
    mode = _math_mode()
    key = ImageKey(id(w), kind, stride, pad, dil, mode, id(bn) if bn is not None else 0)
    ent = _images.get(key)
    if ent is not None and ent.is_for(w, bn):
        if ent.stale(w):
            _refresh_stale(mode)
    else:
        ent = _Image(key, w, bn)
        _build_one(ent, w)
        _images[key] = ent
    return ent.image if (bn is None or kind == 1) else (ent.image, ent.shift)


def _fold_bn(conv, bn):
    """(w * scale[co], shift) with scale = gamma / sqrt(var + eps), shift = beta - mean * scale: a frozen BatchNorm behind
    a frozen convolution is the same convolution with other constants.  Rebuilt only when a tensor's version moves.
    NOT the library-side fold of weight_image(w, 0, bn=bn): that one scales with rsqrtf inside conv_wprep, this one with
    torch.rsqrt in ATen, and nobody has shown that the two give the same bits -- the frozen stages keep theirs."""
    key = (id(conv.weight), id(bn))
    vers = (conv.weight._version, bn.weight._version, bn.bias._version, bn.running_mean._version, bn.running_var._version,
            conv.weight.data_ptr())
    ent = _folded.get(key)
    if ent is None or ent.weight() is not conv.weight or ent.norm() is not bn or ent.versions != vers:
        with torch.no_grad():
            scale = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
            shift = (bn.bias - bn.running_mean * scale).contiguous()
            w = (conv.weight * scale.view(-1, 1, 1, 1)).contiguous(memory_format=torch.channels_last)
        ent = _folded[key] = _Folded(weakref.ref(conv.weight, lambda _, k=key: _folded.pop(k, None)), weakref.ref(bn), vers, w, shift)
    return ent.folded, ent.shift
