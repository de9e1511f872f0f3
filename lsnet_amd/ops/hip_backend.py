"""The 'cuda' (HIP) backend: marshals torch tensors into the C ABI of liblsnet_hip.so."""
import ctypes

import torch

from .. import _lib
from .._lib import ptr, stream
from .._lib import ptr as _ptr, stream as _stream  # noqa: F401  (the names tests/test_ops_gpu.py imports from here)
from .backend import register_backend

_CL = torch.channels_last
# LSNET_CACHE_DCN_IMAGES=0: the deformable layers build their weight images inside every call, as until round 5 (A/B switch)
CACHE_DCN_IMAGES = __import__('os').environ.get('LSNET_CACHE_DCN_IMAGES', '1') != '0'


def _f32(t, what):
    if t.dtype != torch.float32:
        raise TypeError(f'{what} must be float32, got {t.dtype}')
    return t


def _is_nhwc(t):
    return t.dim() == 4 and t.is_contiguous(memory_format=_CL)


def _dense(t, nhwc):
    """offset / mask tensors travel by strides; they only need to be non-overlapping and dense so
    that `empty_like` gives a gradient buffer with identical strides."""
    if t.is_contiguous() or t.is_contiguous(memory_format=_CL):
        return t
    return t.contiguous(memory_format=_CL) if nhwc else t.contiguous()


def _pixel_pitch(t):
    """Floats from one pixel to the next when `t` (B, C, H, W) is a channel slice of a dense channels-last tensor (or a
    dense one itself), else None."""
    if t.dim() != 4 or t.stride(1) != 1:
        return None
    B, C, H, W = t.shape
    p = t.stride(3)
    if p < C or p % 4 or t.stride(2) != W * p or (B > 1 and t.stride(0) != H * W * p):
        return None
    return p


def pool_pitch(t):
    """Floats from one pixel to the next when `t` (B, C, H, W) is a dense channels-last tensor or a channel slice of one --
    what the pooling entry points address by (base, pixel pitch) -- else None.  (Strides of extent-1 axes say nothing.)"""
    if t.dim() != 4 or (t.shape[1] > 1 and t.stride(1) != 1) or t.numel() == 0:
        return None
    B, C, H, W = t.shape
    p = t.stride(3) if W > 1 else t.stride(2) if H > 1 else t.stride(0) if B > 1 else C
    if p < C or (W > 1 and t.stride(3) != p) or (H > 1 and t.stride(2) != W * p) or (B > 1 and t.stride(0) != H * W * p):
        return None
    return p


def _writable(t):
    """a gradient buffer the kernels may write through its strides: fp32 and dense (no two elements at one address)"""
    if t.dtype != torch.float32:
        return False
    expect = 1
    for st, n in sorted((st, n) for st, n in zip(t.stride(), t.shape) if n > 1):
        if st != expect:
            return False
        expect *= n
    return True


def _strides(t):
    s = t.stride()
    return _lib.Strides4(s[0], s[1], s[2], s[3])


class HipBackend:
    name = 'hip'

    # ------------------------------------------------------------------ group norm (+ReLU), channels-last
    @staticmethod
    def group_norm_supported(C, G):
        return C % 4 == 0 and C % G == 0 and ((C // G) % 4 == 0 or 4 % (C // G) == 0) and C // 4 <= 256 and 256 % (C // 4) == 0 and G <= 256

    @staticmethod
    def _gn_levels(xs, ys=None, dys=None, dxs=None):
        n = len(xs)
        levels = (_lib.GnLevel * n)()
        for i, x in enumerate(xs):
            B, C, H, W = x.shape
            L = levels[i]
            L.x = ptr(x)
            L.y = ptr(ys[i]) if ys is not None else None
            L.dy = ptr(dys[i]) if dys is not None else None
            L.dx = ptr(dxs[i]) if dxs is not None else None
            L.B, L.HW = B, H * W
        return levels

    def group_norm_forward(self, xs, gamma, beta, groups, eps, relu, cat_px=False):
        """xs: channels-last (B, C, H, W) tensors sharing gamma/beta.  Returns (ys, mean_rstd).
        cat_px: the outputs are written as the levels of ONE (B, N_all, C) tensor (pixel rows of all levels back to back:
        LSHead._cat_px's layout); ys is then that tensor, viewed as (B, C, N_all, 1)."""
        lib = _lib.load()
        n, C = len(xs), xs[0].shape[1]
        if cat_px:
            B = xs[0].shape[0]
            assert all(x.shape[0] == B for x in xs)
            hw = [x.shape[2] * x.shape[3] for x in xs]
            flat = torch.empty((B, sum(hw), C), device=xs[0].device, dtype=torch.float32)
            ys, o = [], 0
            for k in hw:
                ys.append(flat[:, o:o + k])      # (B, k, C), batch stride N_all * C
                o += k
            levels = self._gn_levels(xs, ys=ys)
            for L in levels:
                L.y_batch_stride = flat.stride(0)
        else:
            ys = [torch.empty_like(x, memory_format=_CL) for x in xs]
            levels = self._gn_levels(xs, ys=ys)
        images = sum(x.shape[0] for x in xs)
        mean_rstd = torch.empty(images, groups, 2, device=xs[0].device, dtype=torch.float32)
        ws = torch.empty(lib.lsn_group_norm_workspace_bytes(n, levels, C, groups), device=xs[0].device,
                         dtype=torch.uint8)
        _lib.check(lib.lsn_group_norm_forward(n, levels, C, groups, ptr(gamma), ptr(beta), eps, 1 if relu else 0,
                                              ptr(mean_rstd), ptr(ws), stream()))
        if cat_px:
            return flat.unsqueeze(2).permute(0, 3, 1, 2), mean_rstd      # (B, C, N_all, 1), channels-last memory
        return ys, mean_rstd

    supports_grad_sinks = True

    def group_norm_backward(self, xs, dys, gamma, beta, groups, relu, mean_rstd, need_params, sinks=None):
        """Returns (dxs, dgamma, dbeta); dgamma/dbeta are None unless need_params.  `sinks` = (dgamma, dbeta) buffers
        to ADD the parameter gradients to (ops/grad_sink.py)."""
        lib = _lib.load()
        n, C = len(xs), xs[0].shape[1]
        dxs = [torch.empty_like(x, memory_format=_CL) for x in xs]
        if torch.is_tensor(dys):     # the gradient of a cat_px output: (B, C, N_all, 1); its levels are read in place
            B = dys.shape[0]
            flat = dys.permute(0, 2, 3, 1).reshape(B, -1, C)
            if not flat.is_contiguous():
                flat = flat.contiguous()
            dyl, o = [], 0
            for x in xs:
                k = x.shape[2] * x.shape[3]
                dyl.append(flat[:, o:o + k])
                o += k
            levels = self._gn_levels(xs, dys=dyl, dxs=dxs)
            for L in levels:
                L.dy_batch_stride = flat.stride(0)
        else:
            dys = [d.contiguous(memory_format=_CL) for d in dys]
            levels = self._gn_levels(xs, dys=dys, dxs=dxs)
        if sinks:
            dg, db = sinks
        else:
            dg = torch.empty_like(gamma) if need_params else None
            db = torch.empty_like(beta) if need_params else None
        ws = torch.empty(lib.lsn_group_norm_workspace_bytes(n, levels, C, groups), device=xs[0].device,
                         dtype=torch.uint8)
        _lib.check(lib.lsn_group_norm_backward(n, levels, C, groups, ptr(gamma), ptr(beta), 1 if relu else 0,
                                               ptr(mean_rstd), ptr(dg), ptr(db), ptr(ws), 1 if sinks else 0, stream()))
        return dxs, dg, db

    # ------------------------------------------------------------------ deformable conv family
    @staticmethod
    def _prep(inputs, offsets, masks, weight):
        nhwc = all(_is_nhwc(x) for x in inputs)
        if nhwc:
            xs = list(inputs)
            w = weight.contiguous(memory_format=_CL)
        else:
            xs = [x.contiguous() for x in inputs]
            w = weight.contiguous()
        offs = [_dense(_f32(o, 'offset'), nhwc) for o in offsets]
        msks = [None if m is None else _dense(_f32(m, 'mask'), nhwc) for m in masks]
        for x in xs:
            _f32(x, 'input')
        _f32(w, 'weight')
        return nhwc, xs, offs, msks, w

    @staticmethod
    def _shape(w, cfg):
        Co, Cg, kh, kw = w.shape
        return _lib.DcnShape(0, Cg * cfg['groups'], 0, 0, Co, 0, 0, kh, kw, cfg['stride'], cfg['pad'],
                             cfg['dil'], cfg['groups'], cfg['dg'], 1.0, 1.0, 1 if cfg.get('fused_om') else 0)

    @staticmethod
    def _mask_view_ptr(om, cfg, kk):
        """Fused DCNv2 pack: `om` (B, 3*dg*K, H, W) holds offsets in its first 2*dg*K channels and the
        mask logits in the rest; the mask pointer is the same buffer advanced by 2*dg*K channels."""
        return om.data_ptr() + 2 * cfg['dg'] * kk * om.stride(1) * om.element_size()

    def _dcn_levels(self, xs, offs, msks, w, cfg, out_hw):
        """The lsn_dcn_level array of a call with its inputs filled in: input / offset / mask pointers and strides (the mask
        of a fused DCNv2 pack is a view of the offsets), sizes and scales.  The caller adds its output or gradient pointers."""
        levels = (_lib.DcnLevel * len(xs))()
        for L, x, off, msk, (Ho, Wo), scale in zip(levels, xs, offs, msks, out_hw, cfg['scales']):
            L.input, L.offset, L.mask = ptr(x), ptr(off), ptr(msk)
            L.off_st = _strides(off)
            if cfg.get('fused_om'):
                L.mask, L.mask_st = self._mask_view_ptr(off, cfg, w.shape[2] * w.shape[3]), _strides(off)
            elif msk is not None:
                L.mask_st = _strides(msk)
            L.B, L.H, L.W, L.Ho, L.Wo = x.shape[0], x.shape[2], x.shape[3], Ho, Wo
            L.scale_h, L.scale_w = scale
        return levels

    @staticmethod
    def _weight_workspace(shape, levels, w, weight, cfg, nhwc, backward):
        """Sets shape.workspace (and weights_prepared) of a split-math call and returns the tensor behind it: the weight's
        fragment image from the per-optimizer-step cache (ops/weight_images.py; kind 0: forward, 2: the backward GEMM) or the
        call's own scratch for the split weight planes.  The cache serves a channels-last PARAMETER handed over as it is (a
        temporary's image would be built and dropped per call), groups = 1, and only after the library said that this call reads
        a prepared image (lsn_dcn_prepared_ok; its routing reads `workspace` as a flag, and in the backward pass needs the gather
        workspace in `shape`): the cache holds no image that no call reads."""
        if CACHE_DCN_IMAGES and nhwc and w is weight and cfg['groups'] == 1 and isinstance(weight, torch.nn.Parameter):
            shape.workspace, shape.weights_prepared = w.data_ptr(), 1
            if _lib.load().lsn_dcn_prepared_ok(ctypes.byref(shape), len(levels), levels, 1 if backward else 0):
                from .weight_images import weight_image
                try:
                    img = weight_image(w, 2 if backward else 0, 1, cfg['pad'], cfg['dil'])
                    shape.workspace = img.data_ptr()
                    return img
                except NotImplementedError:
                    pass
            shape.weights_prepared = 0      # (a cached image must not be written: own scratch)
        ws = torch.empty(2 * w.numel(), device=w.device, dtype=torch.float32)
        shape.workspace = ws.data_ptr()
        return ws

    def dcn_forward(self, inputs, offsets, masks, weight, bias, cfg, out_hw):
        """inputs/offsets/masks: per-level lists (mask entries may be None); cfg: stride, pad, dil,
        groups, dg, scales[(sh, sw)]; out_hw: per-level (Ho, Wo).  Returns the per-level outputs."""
        lib = _lib.load()
        nhwc, xs, offs, msks, w = self._prep(inputs, offsets, masks, weight)
        n = len(xs)
        shape = self._shape(w, cfg)
        levels = self._dcn_levels(xs, offs, msks, w, cfg, out_hw)
        outs = []
        # cfg['concat'] = g: the outputs of g consecutive levels are wanted side by side in ONE (B, g Co, Ho, Wo) tensor (LSHead:
        # the three maps a level gathers, lsnet_head.py:640-647).  The kernels write them there (lsn_dcn_shape.out_pitch)
        # when they can; otherwise the levels get their own buffers and ATen concatenates.
        g = int(cfg.get('concat') or 0)
        Co = w.shape[0]
        wide = None
        if g > 1:
            assert n % g == 0 and all(out_hw[i] == out_hw[i - i % g] and xs[i].shape[0] == xs[i - i % g].shape[0] for i in range(n))
            if nhwc and (g * Co) % 4 == 0:
                wide = [torch.empty((xs[j].shape[0], g * Co) + tuple(out_hw[j]), device=xs[j].device, dtype=torch.float32,
                                    memory_format=_CL) for j in range(0, n, g)]
        for i in range(n):
            if wide is not None:
                out = wide[i // g].narrow(1, (i % g) * Co, Co)
            else:
                out = torch.empty((xs[i].shape[0], Co) + tuple(out_hw[i]), device=xs[i].device, dtype=torch.float32,
                                  memory_format=_CL if nhwc else torch.contiguous_format)
            outs.append(out)
            levels[i].output = ptr(out)
        b = None if bias is None else _f32(bias.contiguous(), 'bias')
        if _lib.split_math():    # the weight's image, or scratch for its pre-split planes (held until the launch)
            ws = self._weight_workspace(shape, levels, w, weight, cfg, nhwc, False)  # noqa: F841
        if wide is not None:
            shape.out_pitch = g * Co
            if not lib.lsn_dcn_pitched_ok(ctypes.byref(shape), n, levels, 0):   # (exact-fp32 mode, odd channel counts)
                shape.out_pitch = 0
                wide = None
                outs = [torch.empty(tuple(o.shape), device=o.device, dtype=torch.float32, memory_format=_CL) for o in outs]
                for i in range(n):
                    levels[i].output = ptr(outs[i])
        _lib.check(lib.lsn_dcn_forward(ctypes.byref(shape), n, levels, ptr(w), ptr(b), 1 if nhwc else 0, stream()))
        if g > 1:
            return wide if wide is not None else [torch.cat(outs[j:j + g], dim=1) for j in range(0, n, g)]
        return outs

    @staticmethod
    def dcn_sinks_ok(inputs, weight):
        """May dcn_backward be handed `sinks` for these tensors?  Only where the kernels write the gradient of `weight` itself:
        channels-last inputs and a weight `_prep` passes on as it is (not a re-laid temporary)."""
        return all(_is_nhwc(x) for x in inputs) and weight.is_contiguous(memory_format=_CL)

    def dcn_backward(self, inputs, offsets, masks, weight, grad_outs, cfg, need, sinks=None):
        """need: dict(input=[bool]*n, offset=[bool]*n, mask=[bool]*n, weight=bool, bias=bool).  sinks: (grad_weight, grad_bias
        or None) buffers to ADD the parameter gradients to (ops/grad_sink.py), for calls that pass `dcn_sinks_ok`.
        Returns (grad_inputs, grad_offsets, grad_masks, grad_weight, grad_bias)."""
        nhwc, xs, offs, msks, w = self._prep(inputs, offsets, masks, weight)
        n = len(xs)
        # channel slices of wider channels-last tensors (the gradient of a concatenation) are read where they lie when the
        # kernels can (lsn_dcn_shape.out_pitch): _dcn_backward_call falls back to dense copies otherwise
        pitches = {_pixel_pitch(g) for g in grad_outs} if nhwc else {None}
        if len(pitches) == 1 and None not in pitches and pitches != {w.shape[0]}:
            gos = list(grad_outs)
        else:
            gos = [(g.contiguous(memory_format=_CL) if nhwc else g.contiguous()) for g in grad_outs]
        gxs, goffs, gmsks = [], [], []
        shared = {}   # levels sampling ONE source map (pyramid op) accumulate into one grad_input buffer
        bufs = []     # per level: the grad_input buffer the kernels write (shared ones appear several times)
        for i in range(n):
            gx = gx_ret = None
            if need['input'][i]:
                key = (xs[i].data_ptr(), tuple(xs[i].shape)) if nhwc else i
                if key in shared:
                    gx = shared[key]            # the first level of the group returns the buffer, the others None
                else:
                    gx = gx_ret = shared[key] = torch.empty_like(xs[i])
            want_om = need['offset'][i] or (msks[i] is not None and need['mask'][i])
            goffs.append(torch.empty_like(offs[i]) if want_om else None)
            gmsks.append(torch.empty_like(msks[i]) if (want_om and msks[i] is not None) else None)
            gxs.append(gx_ret)
            bufs.append(gx)
        if sinks is not None:     # accumulate into the caller's gradient arena
            assert nhwc and w is weight, 'dcn_backward: sinks for a call that dcn_sinks_ok declines'
            gw, gb = sinks
            acc = 1
        else:
            gw = torch.empty_like(w) if (need['weight'] or need['bias']) else None
            gb = torch.empty(w.shape[0], device=w.device, dtype=torch.float32) if need['bias'] else None
            acc = 0
        # (One call per image -- the column gradients of ONE image of a tower launch, 207 MB, fit the 256 MB Infinity Cache,
        # those of the batch, 413 MB, do not -- was measured SLOWER: deformable backward-data 7.6 vs 6.8 ms per step,
        # profiles/r4_per_image.txt: half-size launches lose more to their tails than the cache returns.)
        self._dcn_backward_call(xs, offs, msks, w, gos, bufs, goffs, gmsks, gw, gb, acc, cfg, nhwc, weight)
        return gxs, goffs, gmsks, gw, gb

    def _dcn_backward_call(self, xs, offs, msks, w, gos, gx_bufs, goffs, gmsks, gw, gb, accumulate, cfg, nhwc, weight=None):
        """One lsn_dcn_backward call over the given (level) tensors; every output buffer is the caller's."""
        lib = _lib.load()
        n = len(xs)
        shape = self._shape(w, cfg)
        levels = self._dcn_levels(xs, offs, msks, w, cfg, [g.shape[2:] for g in gos])
        for L, go, gx, goff, gmsk in zip(levels, gos, gx_bufs, goffs, gmsks):
            L.grad_output, L.grad_input, L.grad_offset, L.grad_mask = ptr(go), ptr(gx), ptr(goff), ptr(gmsk)
            if cfg.get('fused_om') and goff is not None:   # one gradient tensor for offsets + mask logits
                L.grad_mask = self._mask_view_ptr(goff, cfg, w.shape[2] * w.shape[3])
        # column-gradient buffer + anchor lists of the atomic-free grad_input path, in every math mode (round 6: the exact mode's
        # column gradients are fmaf chains in front of the same gather; 0 bytes: a shape only the scatter kernels serve)
        nbytes = int(lib.lsn_dcn_backward_workspace_bytes(ctypes.byref(shape), n, levels))
        if nbytes > 0:
            gws = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
            shape.gather_workspace, shape.gather_workspace_bytes = gws.data_ptr(), nbytes
        if cfg['groups'] == 1 and _lib.split_math():    # the weight's image, or scratch for its split + transposed planes
            ws = self._weight_workspace(shape, levels, w, weight, cfg, nhwc, True)  # noqa: F841
        shape.accumulate_param_grads = 1 if accumulate else 0
        pitch = _pixel_pitch(gos[0]) if nhwc else None
        if pitch is not None and pitch != w.shape[0]:
            shape.out_pitch = pitch
            if not lib.lsn_dcn_pitched_ok(ctypes.byref(shape), n, levels, 1):
                shape.out_pitch = 0
                gos = [g.contiguous(memory_format=_CL) for g in gos]
                for i in range(n):
                    levels[i].grad_output = ptr(gos[i])
        _lib.check(lib.lsn_dcn_backward(ctypes.byref(shape), n, levels, ptr(w), ptr(gw), ptr(gb),
                                        1 if nhwc else 0, stream()))

    # ------------------------------------------------------------------ sigmoid focal loss
    @staticmethod
    def _focal_rows(logits, targets, weight=None, d_losses=None):
        """(N, C) of the logits, after checking what the kernels index unchecked: targets[n], weight[n], d_losses[n, c]"""
        if logits.dim() != 2:
            raise ValueError(f'focal loss: logits must be (N, C), got {tuple(logits.shape)}')
        N, C = logits.shape
        if targets.dtype != torch.int64:
            raise TypeError('targets must be int64')
        if targets.numel() != N or targets.device != logits.device:
            raise ValueError(f'focal loss: {targets.numel()} targets on {targets.device} for {N} rows of logits on {logits.device}')
        if weight is not None and (weight.numel() != N or weight.device != logits.device):
            raise ValueError(f'focal loss: {weight.numel()} weights on {weight.device} for {N} rows of logits on {logits.device}')
        if d_losses is not None and (d_losses.shape != logits.shape or d_losses.device != logits.device):
            raise ValueError(f'focal loss: upstream gradient {tuple(d_losses.shape)} for logits {tuple(logits.shape)}')
        return N, C

    def focal_forward(self, logits, targets, gamma, alpha):
        lib = _lib.load()
        logits = _f32(logits, 'logits').contiguous()
        targets = targets.contiguous()
        if targets.dtype != torch.int64:
            raise TypeError('targets must be int64')
        out = torch.empty_like(logits)
        N, C = self._focal_rows(logits, targets)
        _lib.check(lib.lsn_sigmoid_focal_loss_forward(ptr(logits), ptr(targets), ptr(out), N, C, gamma, alpha,
                                                      stream()))
        return out

    def focal_backward(self, logits, targets, d_losses, gamma, alpha):
        lib = _lib.load()
        logits = logits.contiguous()
        d_losses = d_losses.contiguous()
        out = torch.empty_like(logits)
        N, C = self._focal_rows(logits, targets, d_losses=d_losses)
        _lib.check(lib.lsn_sigmoid_focal_loss_backward(ptr(logits), ptr(targets.contiguous()), ptr(d_losses),
                                                       ptr(out), N, C, gamma, alpha, stream()))
        return out

    def focal_sum(self, logits, targets, weight, gamma, alpha):
        lib = _lib.load()
        logits = _f32(logits, 'logits').contiguous()
        out = torch.empty((), device=logits.device, dtype=torch.float32)
        N, C = self._focal_rows(logits, targets, weight)
        w = None if weight is None else _f32(weight, 'weight').contiguous()
        _lib.check(lib.lsn_sigmoid_focal_loss_sum(ptr(logits), ptr(targets.contiguous()), ptr(w), ptr(out), N,
                                                  C, gamma, alpha, stream()))
        return out

    def focal_backward_weighted(self, logits, targets, weight, scale, gamma, alpha):
        lib = _lib.load()
        logits = logits.contiguous()
        out = torch.empty_like(logits)
        N, C = self._focal_rows(logits, targets, weight)
        w = None if weight is None else weight.contiguous()
        scale = scale.to(torch.float32).contiguous()
        _lib.check(lib.lsn_sigmoid_focal_loss_backward_weighted(
            ptr(logits), ptr(targets.contiguous()), ptr(w), ptr(scale), ptr(out), N, C, gamma, alpha, stream()))
        return out

    # ------------------------------------------------------------------ per-level loss sums (LSHead's concatenated rows)
    @staticmethod
    def _level_starts(num_level):
        starts = [0]
        for n in num_level:
            starts.append(starts[-1] + int(n))
        return (ctypes.c_int * len(starts))(*starts), starts[-1]

    def focal_level_sums(self, logits, targets, weight, B, num_level, gamma, alpha):
        """(L,) per-level sums of weight * focal loss over the (B * N_all, C) rows, levels back to back per image."""
        lib = _lib.load()
        assert logits.is_contiguous() and targets.is_contiguous() and (weight is None or weight.is_contiguous())
        _f32(logits, 'logits')
        if targets.dtype != torch.int64:
            raise TypeError('targets must be int64')
        starts, nall = self._level_starts(num_level)
        N, C = logits.shape
        assert N == B * nall and targets.numel() == N
        out = torch.empty(len(num_level), device=logits.device, dtype=torch.float32)
        _lib.check(lib.lsn_sigmoid_focal_loss_level_sums(ptr(logits), ptr(targets), ptr(weight), ptr(out), B, nall, C,
                                                         len(num_level), starts, gamma, alpha, stream()))
        return out

    def focal_backward_levels(self, logits, targets, weight, scales, B, num_level, gamma, alpha):
        lib = _lib.load()
        starts, nall = self._level_starts(num_level)
        N, C = logits.shape
        out = torch.empty_like(logits)
        scales = scales.to(torch.float32).contiguous()
        assert scales.numel() == len(num_level)
        _lib.check(lib.lsn_sigmoid_focal_loss_backward_levels(ptr(logits), ptr(targets), ptr(weight), ptr(scales), ptr(out),
                                                              B, nall, C, len(num_level), starts, gamma, alpha, stream()))
        return out

    def level_sums(self, rows, B, num_level):
        lib = _lib.load()
        starts, nall = self._level_starts(num_level)
        assert rows.is_contiguous() and rows.numel() == B * nall and rows.dtype == torch.float32
        out = torch.empty(len(num_level), device=rows.device, dtype=torch.float32)
        _lib.check(lib.lsn_level_sums(ptr(rows), ptr(out), B, nall, len(num_level), starts, stream()))
        return out

    def level_expand(self, g, B, num_level):
        lib = _lib.load()
        starts, nall = self._level_starts(num_level)
        g = g.to(torch.float32).contiguous()
        out = torch.empty(B * nall, device=g.device, dtype=torch.float32)
        _lib.check(lib.lsn_level_expand(ptr(g), ptr(out), B, nall, len(num_level), starts, stream()))
        return out

    # ------------------------------------------------------------------ NMS
    def nms(self, dets, iou_thr):
        """dets (n,5) float32 on the device -> keep indices (int64), descending score."""
        lib = _lib.load()
        dets = _f32(dets, 'dets').contiguous()
        n = dets.shape[0]
        if n == 0:
            return dets.new_zeros(0, dtype=torch.long)
        order = dets[:, 4].sort(0, descending=True)[1].contiguous()  # nms_kernel.cu:81-83
        keep = torch.empty(n, dtype=torch.int64, device=dets.device)
        num = torch.zeros(1, dtype=torch.int64, device=dets.device)
        ws = torch.empty(int(lib.lsn_nms_workspace_bytes(n)), dtype=torch.uint8, device=dets.device)
        _lib.check(lib.lsn_nms(ptr(dets), ptr(order), n, iou_thr, ptr(keep), ptr(num), ptr(ws), stream()))
        return keep[:int(num.item())]

    # ------------------------------------------------------------------ detection decode
    DECODE_KINDS = {'bbox': 0, 'segm': 1, 'pose_kbox': 1, 'pose_bbox': 2}

    def decode_batch(self, levels, img_hw, scale_factors, num_vectors, kind, nms_pre, score_thr, iou_thr, class_agnostic,
                     max_per_img, cand_cap):
        """LSHead.get_bboxes for a batch in one call (lsn_decode_batch).  levels: (cls (B, C, H, W), box map, vector map,
        stride) per level, float32 device tensors of any strides, read in place; img_hw / scale_factors: per image (h, w) and
        four factors.  -> (dets (B, max_per_img, 5), vecs (B, max_per_img, 2 nv), labels (B, max_per_img) int64, counts (B,)
        int32), all on the device: the first counts[b] rows of image b are its detections; a negative count means more
        than cand_cap candidates -- that image's rows are undefined."""
        lib = _lib.load()
        B, C = levels[0][0].shape[:2]
        dev = levels[0][0].device
        arr = (_lib.DecodeLevel * len(levels))()
        for lv, (cls, box, vec, stride) in zip(arr, levels):
            for t, what in ((cls, 'cls'), (box, 'box map'), (vec, 'vector map')):
                _f32(t, what)
                if t.dim() != 4 or t.shape[0] != B or t.shape[2:] != cls.shape[2:] or t.device != dev:
                    raise ValueError(f'decode_batch: {what} of shape {tuple(t.shape)} beside logits {tuple(cls.shape)}')
            lv.H, lv.W, lv.stride = cls.shape[2], cls.shape[3], float(stride)
            lv.cls, lv.box, lv.vec = cls.data_ptr(), box.data_ptr(), vec.data_ptr()
            lv.cls_strides[:], lv.box_strides[:], lv.vec_strides[:] = cls.stride(), box.stride(), vec.stride()
        hw = (ctypes.c_float * (2 * B))(*[float(v) for p in img_hw for v in p])
        sf = (ctypes.c_float * (4 * B))(*[float(v) for p in scale_factors for v in p])
        nbytes = int(lib.lsn_decode_workspace_bytes(B, len(levels), arr, int(nms_pre), int(cand_cap)))
        if nbytes < 0:
            _lib.check(-1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dets = torch.empty((B, max_per_img, 5), dtype=torch.float32, device=dev)
        vecs = torch.empty((B, max_per_img, 2 * num_vectors), dtype=torch.float32, device=dev)
        labels = torch.empty((B, max_per_img), dtype=torch.int64, device=dev)
        counts = torch.empty((B,), dtype=torch.int32, device=dev)
        _lib.check(lib.lsn_decode_batch(B, len(levels), arr, C, hw, sf, int(num_vectors), int(kind), int(nms_pre), score_thr,
                                        iou_thr, int(bool(class_agnostic)), int(max_per_img), int(cand_cap), dets.data_ptr(),
                                        vecs.data_ptr(), labels.data_ptr(), counts.data_ptr(), ws.data_ptr(), stream()))
        return dets, vecs, labels, counts

    def decode_cpv_batch(self, levels, sources, verify_src, img_hw, scale_factors, nms_pre, score_thr, iou_thr, class_agnostic,
                         max_per_img, cand_cap):
        """LSCPVHead.get_bboxes for a batch in one call (lsn_decode_cpv_batch).  levels: (cls (B, C, H, W), 20-channel
        extreme-point map, stride) per level; sources: (corner heat-map logits (B, 2, H, W), offsets (B, 4, H, W), stride) per
        verification source, each at least 2 x 2; verify_src: per level the index of its source or -1; float32 device
        tensors of any strides, read in place.  -> (dets (B, max_per_img, 5), labels (B, max_per_img) int64, counts (B,)
        int32) as decode_batch returns them."""
        lib = _lib.load()
        B, C = levels[0][0].shape[:2]
        dev = levels[0][0].device

        def same(t, what, like, channels=None):
            _f32(t, what)
            if t.dim() != 4 or t.shape[0] != B or t.shape[2:] != like.shape[2:] or t.device != dev or \
                    (channels is not None and t.shape[1] != channels):
                raise ValueError(f'decode_cpv_batch: {what} of shape {tuple(t.shape)} beside {tuple(like.shape)}')
        arr = (_lib.DecodeLevel * len(levels))()
        for lv, (cls, box, stride) in zip(arr, levels):
            same(cls, 'cls', cls, C)
            same(box, 'box map', cls, 20)
            lv.H, lv.W, lv.stride = cls.shape[2], cls.shape[3], float(stride)
            lv.cls, lv.box, lv.vec = cls.data_ptr(), box.data_ptr(), None
            lv.cls_strides[:], lv.box_strides[:] = cls.stride(), box.stride()
        src = (_lib.DecodeSource * max(1, len(sources)))()
        for sr, (heat, off, stride) in zip(src, sources):
            same(heat, 'corner heat-map', heat, 2)
            same(off, 'corner offsets', heat, 4)
            sr.H, sr.W, sr.stride = heat.shape[2], heat.shape[3], float(stride)
            sr.heat, sr.offset = heat.data_ptr(), off.data_ptr()
            sr.heat_strides[:], sr.offset_strides[:] = heat.stride(), off.stride()
        if len(verify_src) != len(levels):
            raise ValueError(f'decode_cpv_batch: {len(verify_src)} verification entries for {len(levels)} levels')
        verify = (ctypes.c_int * len(levels))(*[int(v) for v in verify_src])
        hw = (ctypes.c_float * (2 * B))(*[float(v) for p in img_hw for v in p])
        sf = (ctypes.c_float * (4 * B))(*[float(v) for p in scale_factors for v in p])
        nbytes = int(lib.lsn_decode_workspace_bytes(B, len(levels), arr, int(nms_pre), int(cand_cap)))
        if nbytes < 0:
            _lib.check(-1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dets = torch.empty((B, max_per_img, 5), dtype=torch.float32, device=dev)
        labels = torch.empty((B, max_per_img), dtype=torch.int64, device=dev)
        counts = torch.empty((B,), dtype=torch.int32, device=dev)
        _lib.check(lib.lsn_decode_cpv_batch(B, len(levels), arr, len(sources), src, verify, C, hw, sf,
                                            int(nms_pre), score_thr, iou_thr, int(bool(class_agnostic)), int(max_per_img),
                                            int(cand_cap), dets.data_ptr(), labels.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                            stream()))
        return dets, labels, counts

    # ------------------------------------------------------------------ k nearest per column (assigners)
    def topk_columns(self, x, k, seg_start, seg_len, largest=False):
        """x (P, G) float32 on the device -> (values, indices), both (nseg * k, G): per row segment the k smallest
        (largest) entries of every column in that order -- torch.topk(x[s:s + n], k, dim=0) of every segment, one launch."""
        lib = _lib.load()
        x = _f32(x, 'x')
        if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
            x = x.contiguous()
        P, G = x.shape
        nseg = len(seg_start)
        vals = torch.empty((nseg * k, G), dtype=torch.float32, device=x.device)
        idx = torch.empty((nseg * k, G), dtype=torch.int64, device=x.device)
        starts = (ctypes.c_int * nseg)(*[int(v) for v in seg_start])
        lens = (ctypes.c_int * nseg)(*[int(v) for v in seg_len])
        _lib.check(lib.lsn_topk_columns(ptr(x), P, G, x.stride(0), nseg, starts, lens, int(k), 1 if largest else 0,
                                        ptr(vals), ptr(idx), stream()))
        return vals, idx

    # ------------------------------------------------------------------ target assignment
    @staticmethod
    def _assign_gts(gt_list, what):
        """list of per-image (G_b, d) tensors -> (rows of all images, host offsets (B + 1), sum G)"""
        offs = [0]
        for t in gt_list:
            offs.append(offs[-1] + t.shape[0])
        rows = gt_list[0] if len(gt_list) == 1 else torch.cat(list(gt_list), 0)
        if what is not None:
            rows = _f32(rows, what)
        return rows.contiguous(), (ctypes.c_int * len(offs))(*offs), offs[-1]

    def centroid_assign_batch(self, points, gt_bboxes, centres, scale, pos_num, gt_labels=None, valid=None, out=None):
        """points (P, 3) shared by the B images; gt_bboxes / centres / gt_labels: lists of B per-image tensors ((G_b, 4),
        (G_b, 2) or None for the box centres, (G_b,) int64 or None).  -> (gt_inds (B, P) int64, labels (B, P) or None).
        `valid`: (B, P) bool / uint8 or None -- the points that exist for each image of a ragged batch; the others are nobody's
        candidates and come out as background (lsn_centroid_assign_masked_batch).
        `out`: preallocated (gt_inds, labels, workspace) for callers that must not allocate (graph capture)."""
        lib = _lib.load()
        points = _f32(points, 'points').contiguous()
        P, B = points.shape[0], len(gt_bboxes)
        gts, offs, G = self._assign_gts(gt_bboxes, 'gt_bboxes')
        cen = None if centres is None else self._assign_gts(centres, 'centres')[0]
        lab = None if gt_labels is None else self._assign_gts(gt_labels, None)[0]
        if lab is not None and lab.dtype != torch.int64:
            raise TypeError(f'gt_labels must be int64, got {lab.dtype}')
        nbytes = int(lib.lsn_assign_workspace_bytes(B * P, G, 1, int(pos_num)))
        if out is None:
            gt_inds = torch.empty((B, P), dtype=torch.int64, device=points.device)
            labels = None if lab is None else torch.empty((B, P), dtype=torch.int64, device=points.device)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=points.device)
        else:
            gt_inds, labels, ws = out
            assert ws.numel() >= nbytes and gt_inds.numel() == B * P and gt_inds.is_contiguous()
        if valid is None:
            _lib.check(lib.lsn_centroid_assign_batch(ptr(points), P, ptr(gts), ptr(cen), B, offs, scale, int(pos_num),
                                                     ptr(lab), ptr(gt_inds), ptr(labels), ptr(ws), stream()))
        else:
            valid = self._u8(valid, (B, P), points.device)
            _lib.check(lib.lsn_centroid_assign_masked_batch(ptr(points), P, ptr(valid), ptr(gts), ptr(cen), B, offs, scale,
                                                            int(pos_num), ptr(lab), ptr(gt_inds), ptr(labels), ptr(ws),
                                                            stream()))
        return gt_inds, labels

    def centroid_assign(self, points, gt_bboxes, centres, scale, pos_num, gt_labels=None, out=None):
        """One image: -> (gt_inds (P,), labels (P,) or None); see centroid_assign_batch."""
        gt_inds, labels = self.centroid_assign_batch(points, [gt_bboxes], None if centres is None else [centres], scale,
                                                     pos_num, None if gt_labels is None else [gt_labels], out=out)
        return gt_inds.view(-1), None if labels is None else labels.view(-1)

    def atss_assign_batch(self, bboxes, level_len, gt_bboxes, topk, gt_labels=None, valid=None, valid_counts=None, out=None):
        """bboxes (B, N, >= 4) float32; level_len: the levels' box counts (sum = N, shared by the images); gt_bboxes /
        gt_labels: lists of B per-image tensors.  -> (gt_inds (B, N), max_overlaps (B, N), labels (B, N) or None).
        `valid`: (B, N) bool / uint8 or None -- the boxes that exist for each image of a ragged batch
        (lsn_atss_assign_masked_batch); `valid_counts`: with it, B lists of HOST ints, the valid boxes per level.  The kernels
        answer a level with fewer than `topk` valid boxes with a shorter candidate list where torch.topk raises: such a
        count is refused here (NotImplementedError), so that the caller's torch path keeps that error.
        `out`: preallocated (gt_inds, max_overlaps, labels, workspace)."""
        lib = _lib.load()
        if valid is not None:
            if valid_counts is None or len(valid_counts) != bboxes.shape[0] or \
                    any(len(c) != len(level_len) for c in valid_counts):
                raise ValueError('atss_assign_batch: a mask needs valid_counts, per image one host integer per level')
            short = [(b, l, int(n)) for b, c in enumerate(valid_counts) for l, n in enumerate(c) if int(n) < int(topk)]
            if short:
                raise NotImplementedError(f'atss_assign_batch: image {short[0][0]} has {short[0][2]} valid boxes on level '
                                          f'{short[0][1]}, topk = {int(topk)}')
        bboxes = _f32(bboxes, 'bboxes')
        if bboxes.stride(2) != 1 or bboxes.stride(1) < bboxes.shape[2] or \
                (bboxes.shape[0] > 1 and bboxes.stride(0) != bboxes.shape[1] * bboxes.stride(1)):
            bboxes = bboxes.contiguous()
        B, N = bboxes.shape[:2]
        gts, offs, G = self._assign_gts(gt_bboxes, 'gt_bboxes')
        assert len(offs) == B + 1
        lab = None if gt_labels is None else self._assign_gts(gt_labels, None)[0]
        if lab is not None and lab.dtype != torch.int64:
            raise TypeError(f'gt_labels must be int64, got {lab.dtype}')
        nlev = len(level_len)
        lens = (ctypes.c_int * nlev)(*[int(v) for v in level_len])
        nbytes = int(lib.lsn_assign_workspace_bytes(B * N, G, nlev, int(topk)))
        if out is None:
            gt_inds = torch.empty((B, N), dtype=torch.int64, device=bboxes.device)
            overlaps = torch.empty((B, N), dtype=torch.float32, device=bboxes.device)
            labels = None if lab is None else torch.empty((B, N), dtype=torch.int64, device=bboxes.device)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=bboxes.device)
        else:
            gt_inds, overlaps, labels, ws = out
            assert ws.numel() >= nbytes and gt_inds.numel() == B * N and gt_inds.is_contiguous() and overlaps.is_contiguous()
        if valid is None:
            _lib.check(lib.lsn_atss_assign_batch(ptr(bboxes), bboxes.stride(1), N, nlev, lens, ptr(gts), B, offs, int(topk),
                                                 ptr(lab), ptr(gt_inds), ptr(overlaps), ptr(labels), ptr(ws), stream()))
        else:
            valid = self._u8(valid, (B, N), bboxes.device)
            _lib.check(lib.lsn_atss_assign_masked_batch(ptr(bboxes), bboxes.stride(1), N, nlev, lens, ptr(valid), ptr(gts), B,
                                                        offs, int(topk), ptr(lab), ptr(gt_inds), ptr(overlaps), ptr(labels),
                                                        ptr(ws), stream()))
        return gt_inds, overlaps, labels

    def atss_assign(self, bboxes, level_len, gt_bboxes, topk, gt_labels=None, out=None):
        """One image, bboxes (N, >= 4): -> (gt_inds (N,), max_overlaps (N,), labels (N,) or None)."""
        gt_inds, overlaps, labels = self.atss_assign_batch(bboxes[None], level_len, [gt_bboxes], topk,
                                                           None if gt_labels is None else [gt_labels], out=out)
        return gt_inds.view(-1), overlaps.view(-1), None if labels is None else labels.view(-1)

    def dense_targets(self, gt_inds, table):
        """gt_inds (P,) int64 (0 = background, k = row k - 1), table (G, D) float32 -> (P, D): the assigned gt's row, zeros
        for background -- torch.where(gt_inds[:, None] > 0, table[gt_inds - 1], 0) in one launch."""
        lib = _lib.load()
        table = _f32(table, 'table').contiguous()
        gt_inds = gt_inds.contiguous()
        if gt_inds.dtype != torch.int64:
            raise TypeError(f'gt_inds must be int64, got {gt_inds.dtype}')
        P, D = gt_inds.numel(), table.shape[1]
        out = torch.empty((P, D), dtype=torch.float32, device=table.device)
        _lib.check(lib.lsn_dense_targets(ptr(gt_inds), P, ptr(table), D, ptr(out), stream()))
        return out

    def assign_targets_batch(self, gt_inds, valid, gt_tables, gt_labels, background_label, out=None):
        """The per-point targets of a stage for all images in one launch (lsn_assign_targets_batch): gt_inds (B, P) int64;
        valid (B, P) bool / uint8 or None; gt_tables: list of B per-image (G_b, D) float32 tables (boxes, then the other target
        fields side by side), an image may have none; gt_labels: list of B (G_b,) int64 tensors or None.
        -> rows (B, P, D), labels (B, P) int64, label_weights (B, P), bbox_weights (B, P, 4), num_pos (B,) int64.
        `out`: these five, preallocated."""
        lib = _lib.load()
        gt_inds = gt_inds.contiguous()
        if gt_inds.dtype != torch.int64 or gt_inds.dim() != 2 or gt_inds.shape[0] != len(gt_tables):
            raise TypeError(f'gt_inds must be int64 (B, P) with one row per table, got {gt_inds.dtype} {tuple(gt_inds.shape)}')
        B, P = gt_inds.shape
        dev = gt_inds.device
        table, offs, G = self._assign_gts(gt_tables, 'gt_tables')
        D = table.shape[1]
        lab = None if gt_labels is None else self._assign_gts(gt_labels, None)[0]
        if lab is not None and (lab.dtype != torch.int64 or lab.numel() != G):
            raise TypeError(f'gt_labels must be int64, one per table row; got {lab.dtype} x {lab.numel()} for {G} rows')
        valid = self._u8(valid, (B, P), dev)
        if out is None:
            rows = torch.empty((B, P, D), dtype=torch.float32, device=dev)
            labels = torch.empty((B, P), dtype=torch.int64, device=dev)
            label_weights = torch.empty((B, P), dtype=torch.float32, device=dev)
            bbox_weights = torch.empty((B, P, 4), dtype=torch.float32, device=dev)
            num_pos = torch.empty((B,), dtype=torch.int64, device=dev)
        else:
            rows, labels, label_weights, bbox_weights, num_pos = out
            assert rows.numel() == B * P * D and labels.numel() == B * P and label_weights.numel() == B * P
            assert bbox_weights.numel() == B * P * 4 and num_pos.numel() == B
            assert all(t.is_contiguous() for t in out) and labels.dtype == torch.int64 and num_pos.dtype == torch.int64
            _f32(rows, 'rows'), _f32(label_weights, 'label_weights'), _f32(bbox_weights, 'bbox_weights')
        _lib.check(lib.lsn_assign_targets_batch(ptr(gt_inds), ptr(valid), P, B, offs, ptr(table), D, ptr(lab),
                                                int(background_label), ptr(rows), ptr(labels), ptr(label_weights),
                                                ptr(bbox_weights), ptr(num_pos), stream()))
        return rows, labels, label_weights, bbox_weights, num_pos

    # ------------------------------------------------------------------ LSHead's point decoding (csrc/points.hip)
    _point_tables = {}

    @classmethod
    def _point_table(cls, picks):
        """the host table of offset sources as the C ABI takes it (kept: the same few tuples come back every step)"""
        t = cls._point_tables.get(picks)
        if t is None:
            t = cls._point_tables[picks] = (ctypes.c_int * len(picks))(*picks)
        return t

    @staticmethod
    def _point_rows(t, what, width=None):
        from .point_decode import row_layout
        lay = row_layout(t) if t.dtype == torch.float32 and t.is_cuda else None
        if lay is None:
            raise ValueError(f'{what}: {tuple(t.shape)} {t.dtype} with strides {t.stride()} is not a tensor of fp32 pixel rows')
        pitch, rows, C = lay
        if width is not None and C != width:
            raise ValueError(f'{what} has rows of {C} floats, expected {width}')
        return ptr(t), pitch, rows, C

    def point_decode_forward(self, raw, n_sp, picks, gradient_mul, base):
        """raw: pixel rows of c_raw floats -> (sp, off) in raw's form (ops/point_decode.py says which forms there are)."""
        from .point_decode import rows_like
        lib = _lib.load()
        rp, rpitch, rows, c_raw = self._point_rows(raw, 'raw')
        n_off = len(picks)
        if base.dtype != torch.float32 or base.device != raw.device or not base.is_contiguous() or base.numel() < n_off:
            raise ValueError(f'base must hold {n_off} contiguous fp32 values on {raw.device}')
        sp, off = rows_like(raw, n_sp), rows_like(raw, n_off)
        _lib.check(lib.lsn_point_decode_forward(rp, rpitch, c_raw, n_sp, self._point_table(picks), n_off, float(gradient_mul),
                                                ptr(base), ptr(sp), n_sp, ptr(off), n_off, rows, stream()))
        return sp, off

    def point_decode_backward(self, raw, sp, n_sp, picks, gradient_mul, g_sp, g_off):
        """The gradient of raw, in raw's form; g_sp / g_off: pixel rows or None."""
        from .point_decode import rows_like
        lib = _lib.load()
        rp, rpitch, rows, c_raw = self._point_rows(raw, 'raw')
        n_off = len(picks)
        sp_p, sp_pitch = self._point_rows(sp, 'sp', n_sp)[:2]
        gs_p, gs_pitch = (None, n_sp) if g_sp is None else self._point_rows(g_sp, 'g_sp', n_sp)[:2]
        go_p, go_pitch = (None, n_off) if g_off is None else self._point_rows(g_off, 'g_off', n_off)[:2]
        g_raw = rows_like(raw, c_raw)
        _lib.check(lib.lsn_point_decode_backward(rp, rpitch, c_raw, n_sp, self._point_table(picks), n_off, float(gradient_mul),
                                                 sp_p, sp_pitch, gs_p, gs_pitch, go_p, go_pitch, ptr(g_raw), c_raw, rows, stream()))
        return g_raw

    def softplus_add_forward(self, a, b):
        from .point_decode import rows_like
        lib = _lib.load()
        ap, apitch, rows, C = self._point_rows(a, 'a')
        bp, bpitch = self._point_rows(b, 'b', C)[:2]
        y = rows_like(a, C)
        _lib.check(lib.lsn_softplus_add_forward(ap, apitch, bp, bpitch, ptr(y), C, C, rows, stream()))
        return y

    def softplus_add_backward(self, a, b, grad_y):
        from .point_decode import rows_like
        lib = _lib.load()
        ap, apitch, rows, C = self._point_rows(a, 'a')
        bp, bpitch = self._point_rows(b, 'b', C)[:2]
        gp, gpitch = self._point_rows(grad_y, 'grad_y', C)[:2]
        ga = rows_like(a, C)
        _lib.check(lib.lsn_softplus_add_backward(ap, apitch, bp, bpitch, gp, gpitch, ptr(ga), C, C, rows, stream()))
        return ga

    POINT_BOX_MODES = {'extreme': 0, 'vectors': 1}

    def point_boxes(self, rows, flat_points, mode, nv):
        """rows (B, N, C), flat_points (N, 3) = x, y, stride -> (B, N, 4) proposal boxes."""
        lib = _lib.load()
        B, N, C = rows.shape
        rp, rpitch = self._point_rows(rows, 'rows')[:2]
        if flat_points.dtype != torch.float32 or tuple(flat_points.shape) != (N, 3) or not flat_points.is_contiguous():
            raise ValueError(f'flat_points must be a contiguous fp32 ({N}, 3) tensor')
        out = torch.empty((B, N, 4), dtype=torch.float32, device=rows.device)
        _lib.check(lib.lsn_point_boxes(rp, rpitch, C, ptr(flat_points), N, B, self.POINT_BOX_MODES[mode], int(nv), ptr(out), 4,
                                       stream()))
        return out

    # ------------------------------------------------------------------ corner-point verification (csrc/cpv.hip)
    @staticmethod
    def _u8(valid, shape, dev):
        if valid is None:
            return None
        if valid.dtype == torch.bool:
            valid = valid.contiguous().view(torch.uint8)
        if valid.dtype != torch.uint8 or tuple(valid.shape) != tuple(shape) or valid.device != dev:
            raise TypeError(f'valid must be a bool / uint8 tensor of shape {tuple(shape)} beside the points')
        return valid.contiguous()

    def corner_targets_batch(self, points, valid, gt_bboxes, gaussian_bump, gaussian_iou, out=None):
        """PointHMAssigner.assign_dense for the B images of a batch over the SAME points (P, 3) in two launches
        (lsn_corner_targets_batch).  valid: (B, P) bool / uint8 or None; gt_bboxes: list of B (G_b, 4) tensors, an image may
        have none.  -> hm (B, 2, P) float32, off (B, 2, P, 2), npos (B, 2) int32; corner 0 = top-left, 1 = bottom-right.
        `out`: preallocated (hm, off, npos, workspace) for callers that must not allocate."""
        lib = _lib.load()
        points = _f32(points, 'points')
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f'points must be (P, 3), got {tuple(points.shape)}')
        points = points.contiguous()
        P, B, dev = points.shape[0], len(gt_bboxes), points.device
        gts, offs, G = self._assign_gts([g[:, :4] for g in gt_bboxes], 'gt_bboxes')
        valid = self._u8(valid, (B, P), dev)
        nbytes = int(lib.lsn_corner_targets_workspace_bytes(G))
        if out is None:
            hm = torch.empty((B, 2, P), dtype=torch.float32, device=dev)
            off = torch.empty((B, 2, P, 2), dtype=torch.float32, device=dev)
            npos = torch.empty((B, 2), dtype=torch.int32, device=dev)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        else:
            hm, off, npos, ws = out
            assert ws.numel() >= nbytes and hm.numel() == B * 2 * P and off.numel() == B * 4 * P and npos.numel() == B * 2
            assert hm.is_contiguous() and off.is_contiguous() and npos.is_contiguous() and npos.dtype == torch.int32
            _f32(hm, 'hm'), _f32(off, 'off')
        _lib.check(lib.lsn_corner_targets_batch(ptr(points), P, ptr(valid), ptr(gts), B, offs, int(bool(gaussian_bump)),
                                                float(gaussian_iou), ptr(hm), ptr(off), ptr(npos), ptr(ws), stream()))
        return hm, off, npos

    def _corner_args(self, scores, offsets, hm, off, valid, npos, grads=None):
        B, dev = scores[0].shape[0], scores[0].device
        arr = (_lib.CornerLevel * len(scores))()
        P = 0
        for i, (lv, s, o) in enumerate(zip(arr, scores, offsets)):
            _f32(s, 'corner scores'), _f32(o, 'corner offsets')
            if s.dim() != 4 or s.shape[:2] != (B, 2) or tuple(o.shape) != (B, 4) + tuple(s.shape[2:]) or o.device != dev:
                raise ValueError(f'corner loss: level {i} has scores {tuple(s.shape)} and offsets {tuple(o.shape)}')
            lv.H, lv.W = s.shape[2], s.shape[3]
            lv.score, lv.offset = s.data_ptr(), o.data_ptr()
            lv.score_strides[:], lv.offset_strides[:] = s.stride(), o.stride()
            if grads is not None:
                gs, go = grads[0][i], grads[1][i]
                assert gs.shape == s.shape and go.shape == o.shape and _writable(gs) and _writable(go)
                lv.grad_score, lv.grad_offset = gs.data_ptr(), go.data_ptr()
                lv.grad_score_strides[:], lv.grad_offset_strides[:] = gs.stride(), go.stride()
            P += lv.H * lv.W
        _f32(hm, 'hm'), _f32(off, 'off')
        if tuple(hm.shape) != (B, 2, P) or tuple(off.shape) != (B, 2, P, 2) or tuple(npos.shape) != (B, 2) or \
                npos.dtype != torch.int32 or not (hm.is_contiguous() and off.is_contiguous() and npos.is_contiguous()):
            raise ValueError(f'corner loss: targets {tuple(hm.shape)} / {tuple(off.shape)} / {tuple(npos.shape)} for {B} images '
                             f'of {P} points')
        return arr, B, P, self._u8(valid, (B, P), dev)

    def corner_loss_forward(self, scores, offsets, hm, off, valid, npos, alpha, gamma, beta, out=None):
        """Corner heat-map (Gaussian focal, on logits) and offset (smooth L1) losses of all levels in two launches.  scores /
        offsets: per level (B, 2, H, W) / (B, 4, H, W), any strides; hm / off / npos / valid: corner_targets_batch's.
        -> (loss_heat (L,), loss_off (L,)), each (S_tl / n_tl + S_br / n_br) / 2.  `out`: (loss_heat, loss_off, workspace)."""
        lib = _lib.load()
        arr, B, P, valid = self._corner_args(scores, offsets, hm, off, valid, npos)
        dev, L = hm.device, len(scores)
        nbytes = int(lib.lsn_corner_loss_workspace_bytes(B, L, arr))
        if out is None:
            heat = torch.empty(L, dtype=torch.float32, device=dev)
            offl = torch.empty(L, dtype=torch.float32, device=dev)
            ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        else:
            heat, offl, ws = out
            assert ws.numel() * ws.element_size() >= nbytes and heat.numel() == L and offl.numel() == L
        _lib.check(lib.lsn_corner_loss_forward(B, P, L, arr, ptr(hm), ptr(off), ptr(valid), ptr(npos), alpha, gamma, beta,
                                               ptr(heat), ptr(offl), ptr(ws), stream()))
        return heat, offl

    def corner_loss_backward(self, scores, offsets, hm, off, valid, npos, alpha, gamma, beta, g_heat, g_off, out=None):
        """-> (grad_scores, grad_offsets), lists of dense tensors in the maps' memory order, every element written, one launch.
        g_heat / g_off: (L,) upstream gradients on the device.  `out`: preallocated (grad_scores, grad_offsets)."""
        lib = _lib.load()
        grads = out if out is not None else ([torch.empty_like(s) for s in scores], [torch.empty_like(o) for o in offsets])
        arr, B, P, valid = self._corner_args(scores, offsets, hm, off, valid, npos, grads)
        g_heat, g_off = _f32(g_heat, 'g_heat').contiguous(), _f32(g_off, 'g_off').contiguous()
        assert g_heat.numel() == len(scores) and g_off.numel() == len(scores)
        _lib.check(lib.lsn_corner_loss_backward(B, P, len(scores), arr, ptr(hm), ptr(off), ptr(valid), ptr(npos), alpha,
                                                gamma, beta, ptr(g_heat), ptr(g_off), stream()))
        return grads

    @staticmethod
    def _sem_args(logits, target, weight, grads=None):
        B, C = logits[0].shape[:2]
        dev = logits[0].device
        _f32(target, 'gt_sem_map'), _f32(weight, 'gt_sem_weights')
        if target.dim() != 4 or target.shape[:2] != (B, C) or weight.shape != target.shape or target.device != dev or \
                weight.device != dev:
            raise ValueError(f'sep focal: semantic maps {tuple(target.shape)} / {tuple(weight.shape)} beside logits of '
                             f'{B} x {C} maps')
        arr = (_lib.SemLevel * len(logits))()
        for i, (lv, x) in enumerate(zip(arr, logits)):
            _f32(x, 'semantic logits')
            if x.dim() != 4 or x.shape[:2] != (B, C) or x.device != dev:
                raise ValueError(f'sep focal: level {i} has logits {tuple(x.shape)}')
            lv.H, lv.W, lv.logits = x.shape[2], x.shape[3], x.data_ptr()
            lv.strides[:] = x.stride()
            if grads is not None:
                assert grads[i].shape == x.shape and _writable(grads[i])
                lv.grad = grads[i].data_ptr()
                lv.grad_strides[:] = grads[i].stride()
        return arr, B, C, target.contiguous(), weight.contiguous()

    def sep_focal_forward(self, logits, target, weight, gamma, alpha, out=None):
        """SEPFocalLoss over the per-level (B, C, H, W) logits against the (B, C, h, w) maps read through the nearest rule of
        F.interpolate, two launches.  -> (loss (1,), stats (4,)): sum_pos / sum_pos(w) + sum_neg / count(target > 0) and what
        backward needs.  `out`: preallocated (loss, stats, workspace)."""
        lib = _lib.load()
        arr, B, C, target, weight = self._sem_args(logits, target, weight)
        dev = target.device
        nbytes = int(lib.lsn_sep_focal_workspace_bytes(B, C, len(logits), arr))
        if out is None:
            loss = torch.empty(1, dtype=torch.float32, device=dev)
            stats = torch.empty(4, dtype=torch.float32, device=dev)
            ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        else:
            loss, stats, ws = out
            assert ws.numel() * ws.element_size() >= nbytes and loss.numel() == 1 and stats.numel() == 4
        _lib.check(lib.lsn_sep_focal_forward(B, C, len(logits), arr, ptr(target), ptr(weight), target.shape[2], target.shape[3],
                                             gamma, alpha, ptr(loss), ptr(stats), ptr(ws), stream()))
        return loss, stats

    def sep_focal_backward(self, logits, target, weight, gamma, alpha, stats, g, out=None):
        """-> list of dense gradients in the logits' memory order, every element written, one launch.  g: the upstream
        gradient (1 element, device).  `out`: the preallocated gradients."""
        lib = _lib.load()
        grads = out if out is not None else [torch.empty_like(x) for x in logits]
        arr, B, C, target, weight = self._sem_args(logits, target, weight, grads)
        g = _f32(g, 'g').reshape(1).contiguous()
        _lib.check(lib.lsn_sep_focal_backward(B, C, len(logits), arr, ptr(target), ptr(weight), target.shape[2],
                                              target.shape[3], gamma, alpha, ptr(stats), ptr(g), stream()))
        return grads

    # ------------------------------------------------------------------ pooling family (csrc/pool.hip), channels-last
    CORNER_MODES = {'top': 0, 'bottom': 1, 'left': 2, 'right': 3}

    @staticmethod
    def _pool_arg(t, what):
        p = pool_pitch(_f32(t, what))
        if p is None:
            raise ValueError(f'{what}: {tuple(t.shape)} with strides {t.stride()} is not (a channel slice of) a channels-last tensor')
        return ptr(t), p

    @staticmethod
    def _pool_new(like, shape):
        return torch.empty(tuple(shape), device=like.device, dtype=torch.float32, memory_format=_CL)

    @staticmethod
    def pool_output_size(n, k, stride, pad, ceil_mode=False):
        return _lib.load().lsn_pool_output_size(n, k, stride, pad, 1 if ceil_mode else 0)

    def max_pool2d_forward(self, x, kernel, stride, pad, want_slot=True, out=None):
        """x (B, C, H, W) channels-last (or a channel slice of such a tensor) -> (y, slot); slot: (B, Ho, Wo, C) uint8, the
        winning window positions the backward needs (None when not wanted)."""
        lib = _lib.load()
        B, C, H, W = x.shape
        kh, kw = kernel
        Ho, Wo = (self.pool_output_size(n, k, stride, pad) for n, k in ((H, kh), (W, kw)))
        y = self._pool_new(x, (B, C, max(Ho, 1), max(Wo, 1))) if out is None else out
        slot = torch.empty((B, max(Ho, 1), max(Wo, 1), C), device=x.device, dtype=torch.uint8) if want_slot else None
        (xp, xpitch), (yp, ypitch) = self._pool_arg(x, 'x'), self._pool_arg(y, 'y')
        _lib.check(lib.lsn_max_pool2d_forward(xp, xpitch, yp, ypitch, ptr(slot), B, H, W, C, kh, kw, stride, pad, stream()))
        return y, slot

    def max_pool2d_backward(self, grad_y, slot, x_shape, kernel, stride, pad, out=None):
        lib = _lib.load()
        B, C, H, W = x_shape
        gx = self._pool_new(grad_y, x_shape) if out is None else out
        (gp, gpitch), (xp, xpitch) = self._pool_arg(grad_y, 'grad_y'), self._pool_arg(gx, 'grad_x')
        _lib.check(lib.lsn_max_pool2d_backward(gp, gpitch, ptr(slot), xp, xpitch, B, H, W, C, kernel[0], kernel[1], stride,
                                               pad, stream()))
        return gx

    def avg_pool2d_forward(self, x, kernel, stride, pad, ceil_mode, count_include_pad, out=None):
        lib = _lib.load()
        B, C, H, W = x.shape
        kh, kw = kernel
        Ho, Wo = (self.pool_output_size(n, k, stride, pad, ceil_mode) for n, k in ((H, kh), (W, kw)))
        y = self._pool_new(x, (B, C, max(Ho, 1), max(Wo, 1))) if out is None else out
        (xp, xpitch), (yp, ypitch) = self._pool_arg(x, 'x'), self._pool_arg(y, 'y')
        _lib.check(lib.lsn_avg_pool2d_forward(xp, xpitch, yp, ypitch, B, H, W, C, kh, kw, stride, pad, 1 if ceil_mode else 0,
                                              1 if count_include_pad else 0, stream()))
        return y

    def avg_pool2d_backward(self, grad_y, x_shape, kernel, stride, pad, ceil_mode, count_include_pad, out=None):
        lib = _lib.load()
        B, C, H, W = x_shape
        gx = self._pool_new(grad_y, x_shape) if out is None else out
        (gp, gpitch), (xp, xpitch) = self._pool_arg(grad_y, 'grad_y'), self._pool_arg(gx, 'grad_x')
        _lib.check(lib.lsn_avg_pool2d_backward(gp, gpitch, xp, xpitch, B, H, W, C, kernel[0], kernel[1], stride, pad,
                                               1 if ceil_mode else 0, 1 if count_include_pad else 0, stream()))
        return gx

    def upsample_add_forward(self, top, lat, out=None):
        """lat + nearest-upsampled top, for lat of twice top's size (or one less, per axis); out may be lat itself."""
        lib = _lib.load()
        B, C, H, W = lat.shape
        h, w = top.shape[2:]
        out = self._pool_new(lat, lat.shape) if out is None else out
        (tp, tpitch), (lp, lpitch), (op, opitch) = self._pool_arg(top, 'top'), self._pool_arg(lat, 'lat'), self._pool_arg(out, 'out')
        _lib.check(lib.lsn_upsample_add_forward(tp, tpitch, lp, lpitch, op, opitch, B, h, w, H, W, C, stream()))
        return out

    def upsample_add_backward(self, grad_out, top_shape, out=None, accumulate=False):
        """The gradient of `top`; accumulate: added to what `out` holds."""
        lib = _lib.load()
        B, C, H, W = grad_out.shape
        h, w = top_shape[2:]
        assert out is not None or not accumulate
        gt = self._pool_new(grad_out, top_shape) if out is None else out
        (gp, gpitch), (tp, tpitch) = self._pool_arg(grad_out, 'grad_out'), self._pool_arg(gt, 'grad_top')
        _lib.check(lib.lsn_upsample_add_backward(gp, gpitch, tp, tpitch, 1 if accumulate else 0, B, h, w, H, W, C, stream()))
        return gt

    def corner_pool_forward(self, mode, x, out=None, accumulate=False):
        """Running maximum of x towards the `mode` border ('top', 'bottom', 'left', 'right'); accumulate: added to `out`."""
        lib = _lib.load()
        B, C, H, W = x.shape
        assert out is not None or not accumulate
        y = self._pool_new(x, x.shape) if out is None else out
        (xp, xpitch), (yp, ypitch) = self._pool_arg(x, 'x'), self._pool_arg(y, 'y')
        _lib.check(lib.lsn_corner_pool_forward(self.CORNER_MODES[mode], xp, xpitch, yp, ypitch, 1 if accumulate else 0, B, H, W, C,
                                               stream()))
        return y

    def corner_pool_backward(self, mode, x, grad_y, out=None, accumulate=False):
        lib = _lib.load()
        B, C, H, W = x.shape
        assert out is not None or not accumulate
        gx = self._pool_new(x, x.shape) if out is None else out
        (xp, xpitch), (gp, gpitch), (dp, dpitch) = self._pool_arg(x, 'x'), self._pool_arg(grad_y, 'grad_y'), self._pool_arg(gx, 'grad_x')
        _lib.check(lib.lsn_corner_pool_backward(self.CORNER_MODES[mode], xp, xpitch, gp, gpitch, dp, dpitch, 1 if accumulate else 0,
                                                B, H, W, C, stream()))
        return gx

    # ------------------------------------------------------------------ LSHead's cumulative offset rescaling
    @staticmethod
    def offset_chain_ok(off):
        """(B, C, H, W) fp32 with channels innermost and pixels back to back inside an image (any image pitch)."""
        if not (off.is_cuda and off.dtype == torch.float32 and off.dim() == 4 and off.shape[1] % 2 == 0):
            return False
        B, C, H, W = off.shape
        return off.stride(1) == 1 and off.stride(3) == C and (H == 1 or off.stride(2) == W * C) and \
            (B == 1 or off.stride(0) >= H * W * C)

    def offset_chain(self, offs, mults):
        """offs: per-level offset fields; mults[l] = ((sh, sw) x 3) -> per level the three rescaled fields."""
        lib = _lib.load()
        n, C = len(offs), offs[0].shape[1]
        lv = (_lib.OffsetChainLevel * n)()
        res = []
        for l, off in enumerate(offs):
            B, _, H, W = off.shape
            L = lv[l]
            L.images, L.per_image = B, H * W * C
            L.off, L.off_image_pitch = ptr(off), (off.stride(0) if B > 1 else H * W * C)
            outs = [torch.empty((B, C, H, W), device=off.device, dtype=torch.float32, memory_format=_CL) for _ in range(3)]
            for k in range(3):
                L.mh[k], L.mw[k] = mults[l][k]
                L.out[k] = outs[k].data_ptr()
            res.append(outs)
        _lib.check(lib.lsn_offset_chain_forward(n, lv, C, stream()))
        return res

    def offset_chain_backward(self, shapes, device, mults, grads):
        """grads[l]: the gradients of level l's three fields, then (optionally) of a second consumer's aliases of them --
        3 or 6 entries, any of them None -> per level the offset field's gradient."""
        lib = _lib.load()
        n, C = len(shapes), shapes[0][1]
        lv = (_lib.OffsetChainLevel * n)()
        keep, res = [], []
        for l, (B, _, H, W) in enumerate(shapes):
            L = lv[l]
            L.images, L.per_image = B, H * W * C
            for k in range(3):
                L.mh[k], L.mw[k] = mults[l][k]
            for k, g in enumerate(grads[l]):
                if g is not None:
                    g = _f32(g, 'grad').contiguous(memory_format=_CL)
                    keep.append(g)
                    L.gout[k] = g.data_ptr()
            goff = torch.empty((B, C, H, W), device=device, dtype=torch.float32, memory_format=_CL)
            L.goff = goff.data_ptr()
            res.append(goff)
        _lib.check(lib.lsn_offset_chain_backward(n, lv, C, stream()))
        return res

    def selftest_mfma(self, A, B, variant):
        lib = _lib.load()
        A, B = A.contiguous(), B.contiguous()
        M, K = A.shape
        N = B.shape[1]
        D = torch.empty(M, N, device=A.device, dtype=torch.float32)
        _lib.check(lib.lsn_selftest_mfma(ptr(A), ptr(B), ptr(D), M, N, K, variant, stream()))
        return D


_lib.load()  # fail loudly at registration time when the library is missing
register_backend('cuda', HipBackend())
