"""Deformable calls whose kernel is not 3 x 3, shared by tests/test_dcn_kernel_sizes_host.py (the oracle against a float64
restatement) and tests/test_dcn_kernel_sizes_gpu.py (the HIP kernels against the oracle).

Every kernel of the deformable family is written for a general kh x kw and keeps the KD = kh kw dg sampling positions of each pixel
of its tile in LDS; which kernel serves a pass follows from KD through the LDS thresholds of csrc/dcn_route.h.  The cases reach
each tap-count-dependent piece at a KD other than 9, 18 or 36: a single (tap, slab) chunk, 25 / 49 / 50 / 64 taps, even and
non-square kernels, the K > 9 exclusion of the grouped weight gradient, and the documented bound of 64 from both sides.

Maps stay at or below 13 x 21 and the reduction depth (C / groups) kh kw at or below 4608 -- the deepest case of
tests/test_ops_gpu.py (r101_l4_s2) -- so that file's TOL = 1e-4 of the reference's range holds here unchanged."""
import functools
import os
import re

import numpy as np
import torch

from oracle import oracle_py as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [
    # name, k = (kh, kw), channels, geometry; like DCN_CASES of tests/test_ops_gpu.py: mask=True and bias=True unless stated
    dict(name='k1_one_chunk', k=(1, 1), pad=0, C=32, Co=128, hw=(9, 14)),             # FWD_MM with one (tap, slab) chunk
    dict(name='k1_wgmm', k=(1, 1), pad=0, C=64, Co=256, hw=(9, 14)),                  # WG_MM with K = 1
    dict(name='k1_c6', k=(1, 1), pad=0, C=6, Co=10, hw=(7, 9)),                       # C % 4 != 0: scalar weight path
    dict(name='k5_pyr', k=(5, 5), pad=2, C=128, Co=256, mask=False, hw=(13, 21), dst=(7, 11)),   # LSHead with 25 kernel points
    dict(name='k5_dg2', k=(5, 5), pad=2, C=64, Co=128, dg=2, hw=(9, 12)),             # KD = 50: no mm / xn tap table fits
    dict(name='k5_g8', k=(5, 5), pad=2, C=64, Co=64, groups=8, hw=(9, 12)),           # FWD_GROUPED; K > 9: split weight gradient
    dict(name='k2_g8', k=(2, 2), pad=1, C=64, Co=64, groups=8, hw=(8, 12)),           # even kernel; WG_GROUPED with K = 4
    dict(name='k1x3_tails', k=(1, 3), pad=1, C=40, Co=72, hw=(9, 14)),                # channel tails
    dict(name='k3x1_s2_g4_dg2', k=(3, 1), stride=2, pad=0, C=16, Co=24, groups=4, dg=2, hw=(13, 21)),
    dict(name='k7_narrow', k=(7, 7), pad=3, C=32, Co=48, hw=(9, 12)),                 # KD = 49
    dict(name='k7_dil2', k=(7, 7), pad=6, dil=2, C=16, Co=24, hw=(13, 21)),
    dict(name='k8_bound', k=(8, 8), pad=3, C=32, Co=32, mask=False, hw=(9, 12)),      # KD = 64, narrow output
    dict(name='k4_dg4_bound', k=(4, 4), pad=1, C=64, Co=128, dg=4, hw=(9, 12)),       # KD = 64, wide output
    dict(name='k5_dg3_over', k=(5, 5), pad=2, C=48, Co=48, dg=3, hw=(7, 9)),          # KD = 75: refused
]
NAMES = [c['name'] for c in CASES]


def case(name):
    return next(c for c in CASES if c['name'] == name)


def kd(c):
    return c['k'][0] * c['k'][1] * c.get('dg', 1)


def make(c, seed=0):
    """_make of tests/test_ops_gpu.py for a kh x kw kernel: B = 2, offsets uniform in [-3, 3) (samples leave the map), weights scaled
    by 1 / sqrt(K C / groups), (Ho, Wo) from orc.out_size per axis or the pyramid's destination grid.  The pyramid scales are
    rounded to fp32 here, so that every consumer -- the C ABI takes floats -- computes with the same numbers."""
    g = torch.Generator().manual_seed(seed)
    B, C, Co = 2, c['C'], c['Co']
    kh, kw = c['k']
    groups, dg = c.get('groups', 1), c.get('dg', 1)
    stride, pad, dil = c.get('stride', 1), c.get('pad', 1), c.get('dil', 1)
    Hs, Ws = c['hw']
    if 'dst' in c:
        Ho, Wo = c['dst']
        sh, sw = float(np.float32(Hs / Ho)), float(np.float32(Ws / Wo))
        pyramid = True
    else:
        Ho, Wo = orc.out_size(Hs, kh, stride, pad, dil), orc.out_size(Ws, kw, stride, pad, dil)
        sh = sw = 1.0
        pyramid = False
    has_mask = c.get('mask', True)
    K = kh * kw
    x = torch.randn(B, C, Hs, Ws, generator=g)
    w = torch.randn(Co, C // groups, kh, kw, generator=g) * (1.0 / (K * (C // groups)) ** 0.5)
    b = torch.randn(Co, generator=g) if (has_mask and c.get('bias', True)) else None
    off = torch.rand(B, dg * 2 * K, Ho, Wo, generator=g) * 6 - 3
    mask = torch.rand(B, dg * K, Ho, Wo, generator=g) if has_mask else None
    go = torch.randn(B, Co, Ho, Wo, generator=g)
    cfg = dict(stride=stride, pad=pad, dil=dil, groups=groups, dg=dg, sh=sh, sw=sw, pyramid=pyramid, out_hw=(Ho, Wo))
    return x, w, b, off, mask, go, cfg


@functools.lru_cache(maxsize=None)
def reference(name):
    """(inputs of make, oracle output, oracle gradients) of a case, computed once and shared; nobody writes to them."""
    made = make(case(name))
    x, w, b, off, mask, go, cfg = made
    out = orc.deform_conv_forward(x, w, b, off, mask, cfg['stride'], cfg['pad'], cfg['dil'], cfg['groups'], cfg['dg'], cfg['sh'],
                                  cfg['sw'], out_hw=cfg['out_hw'])
    grads = orc.deform_conv_backward(x, w, off, mask, go, cfg['stride'], cfg['pad'], cfg['dil'], cfg['groups'], cfg['dg'], cfg['sh'],
                                     cfg['sw'])
    return made, out, grads


def kd_every_route():
    """LSN_DCN_KD_EVERY_ROUTE of include/lsnet_hip.h: the largest kh kw dg that every route of both passes serves."""
    text = open(os.path.join(ROOT, 'include', 'lsnet_hip.h')).read()
    return int(re.search(r'#define\s+LSN_DCN_KD_EVERY_ROUTE\s+(\d+)', text).group(1))


# ---------------------------------------------------------------------------------------------------------------- routes
# The route of every case under the five kernel choices of tests/test_ops_gpu.py (KERNEL_CHOICES), for one channels-last level
# that asks for every gradient, with the workspaces HipBackend passes (`workspace` in the split modes -- backward: groups = 1
# only -- and a gather workspace of the size the library asks for).  Derived by hand from csrc/dcn_route.h; the GPU test checks
# what the C ABI lets one observe of it (lsn_dcn_prepared_ok forward == FWD_MM, backward == GATHER_MM; a gather workspace size
# above zero == a GATHER_* route).  With npl = 3 / 2 / 0 bf16 planes per operand in bf16x6 / bf16x3 / fp32:
#   FWD_MM         split mode, groups = 1, not under DBG_GENERAL_GEMMS, 32 | C / dg, 128 | Co,
#                  fwd_mm_lds = 8192 npl + 2048 KD <= 80 KiB                                  -> KD <= 28 (x6), 32 (x3)
#   FWD_GROUPED    groups > 1, Co = C, C / groups in {8, 16, 32}, 64 | C / dg, 17408 + 1024 K <= 64 KiB    -> K <= 47
#   FWD_XN(_PLANES) split mode, Co / groups > 64, 4 | channel counts, xn_lds = 40960 npl + 2048 KD <= 160 KiB
#                                                                                             -> KD <= 20 (x6), 40 (x3)
#   FWD_FP32       everything else: fwd_fp32_lds = 132 (64 + BN) + 2048 KD with BN = 256 where Co / groups > 64 and it fits
#                  (KD <= 59), else 64 (KD <= 71): serves every KD <= 64
#   GATHER_GROUPED groups > 1 or fp32 mode; 4 | C / groups, 4 | C / dg; not under DBG_ATOMIC_SCATTER
#   GATHER_MM      split mode, groups = 1, `workspace`, 4 | C, 4 | Co, not under DBG_GENERAL_GEMMS / DBG_ATOMIC_SCATTER, the
#                  fragment image of the transposed weight within 8 bytes per weight element:
#                  ceil(Co / 32) nt(K C) 2048 npl <= 8 Co K C, nt(n) = 1, 2 (n <= 32, 64), else 4 ceil(n / 128)
#                  (k7_narrow, bf16x6: 2 x 52 x 6144 = 638976 > 8 x 48 x 49 x 32 = 602112; bf16x3: 425984 fits)
#   GATHER_XN / SCATTER_XN   split mode, groups = 1, `workspace`, Co <= 256, 8 | Co, 4 | C,
#                  bwd_xn_lds = 16384 npl + 2816 KD <= 80 KiB                                 -> KD <= 11 (x6), 17 (x3)
#                  (GATHER_XN with a gather workspace and not under DBG_ATOMIC_SCATTER, else SCATTER_XN)
#   SCATTER_FP32   everything else: bwd_fp32_lds = 128 RED + 2816 KD with RED = 256 where Co / groups > 64 and it fits
#                  (KD <= 46), else 64 (KD <= 55 = LSN_DCN_KD_EVERY_ROUTE); above: refused
#   WG_GROUPED     groups > 1, Co = C, K <= 9, C / groups in {4, 8, 16, 32}, ...
#   WG_MM          the conditions of FWD_MM without the LDS one, 256 | Co, 64 | C / dg, behind a GATHER_* route
#   WG_XN_ORDERED / WG_FP32_ORDERED   everything else in a split mode / in fp32 mode (the partial gradients of these cases fit)
_SPLIT_CHOICES = ('default', 'x6_first_gemms', 'x3_gather', 'x3_atomic_fallbacks')


def _routes(default, first_gemms, x3_gather, x3_atomic, math_fp32):
    return dict(zip(_SPLIT_CHOICES + ('math_fp32',), (default, first_gemms, x3_gather, x3_atomic, math_fp32)))


ROUTES = {
    'k1_one_chunk': _routes(('FWD_MM', 'GATHER_MM', 'WG_XN_ORDERED'), ('FWD_XN_PLANES', 'GATHER_XN', 'WG_XN_ORDERED'),
                            ('FWD_MM', 'GATHER_MM', 'WG_XN_ORDERED'), ('FWD_MM', 'SCATTER_XN', 'WG_XN_ORDERED'),
                            ('FWD_FP32', 'GATHER_GROUPED', 'WG_FP32_ORDERED')),
    'k1_wgmm': _routes(('FWD_MM', 'GATHER_MM', 'WG_MM'), ('FWD_XN_PLANES', 'GATHER_XN', 'WG_XN_ORDERED'),
                       ('FWD_MM', 'GATHER_MM', 'WG_MM'), ('FWD_MM', 'SCATTER_XN', 'WG_XN_ORDERED'),
                       ('FWD_FP32', 'GATHER_GROUPED', 'WG_FP32_ORDERED')),
    'k1_c6': _routes(*[('FWD_FP32', 'SCATTER_FP32', 'WG_XN_ORDERED')] * 4, ('FWD_FP32', 'SCATTER_FP32', 'WG_FP32_ORDERED')),
    # KD = 25: x6 xn_lds = 174080 and bwd_xn_lds = 119552 are over their caps, so DBG_GENERAL_GEMMS ends at the fp32 kernels
    'k5_pyr': _routes(('FWD_MM', 'GATHER_MM', 'WG_MM'), ('FWD_FP32', 'SCATTER_FP32', 'WG_XN_ORDERED'),
                      ('FWD_MM', 'GATHER_MM', 'WG_MM'), ('FWD_MM', 'SCATTER_FP32', 'WG_XN_ORDERED'),
                      ('FWD_FP32', 'GATHER_GROUPED', 'WG_FP32_ORDERED')),
    # KD = 50: over every forward cap but the fp32 kernel's (256-wide: 42240 + 102400); the scatter takes the 64-wide slab
    'k5_dg2': _routes(('FWD_FP32', 'GATHER_MM', 'WG_XN_ORDERED'), ('FWD_FP32', 'SCATTER_FP32', 'WG_XN_ORDERED'),
                      ('FWD_FP32', 'GATHER_MM', 'WG_XN_ORDERED'), ('FWD_FP32', 'SCATTER_FP32', 'WG_XN_ORDERED'),
                      ('FWD_FP32', 'GATHER_GROUPED', 'WG_FP32_ORDERED')),
    'k5_g8': _routes(*[('FWD_GROUPED', 'GATHER_GROUPED', 'WG_XN_ORDERED')] * 3, ('FWD_GROUPED', 'SCATTER_FP32', 'WG_XN_ORDERED'),
                     ('FWD_GROUPED', 'GATHER_GROUPED', 'WG_FP32_ORDERED')),
    'k2_g8': _routes(*[('FWD_GROUPED', 'GATHER_GROUPED', 'WG_GROUPED')] * 3, ('FWD_GROUPED', 'SCATTER_FP32', 'WG_GROUPED'),
                     ('FWD_GROUPED', 'GATHER_GROUPED', 'WG_GROUPED')),
    # C / dg = 40 is no multiple of 32, Co = 72 none of 128: never FWD_MM.  bf16x6: the image of the transposed weight,
    # 3 x 4 x 6144 = 73728, is over 8 x 72 x 3 x 40 = 69120, so GATHER_XN; bf16x3: 49152 fits, GATHER_MM
    'k1x3_tails': _routes(('FWD_XN_PLANES', 'GATHER_XN', 'WG_XN_ORDERED'), ('FWD_XN_PLANES', 'GATHER_XN', 'WG_XN_ORDERED'),
                          ('FWD_XN_PLANES', 'GATHER_MM', 'WG_XN_ORDERED'), ('FWD_XN_PLANES', 'SCATTER_XN', 'WG_XN_ORDERED'),
                          ('FWD_FP32', 'GATHER_GROUPED', 'WG_FP32_ORDERED')),
    'k3x1_s2_g4_dg2': _routes(*[('FWD_FP32', 'GATHER_GROUPED', 'WG_XN_ORDERED')] * 3, ('FWD_FP32', 'SCATTER_FP32', 'WG_XN_ORDERED'),
                              ('FWD_FP32', 'GATHER_GROUPED', 'WG_FP32_ORDERED')),
    # KD = 49 <= 55: the fp32 scatter serves it (64-wide: 8192 + 137984)
    'k7_narrow': _routes(('FWD_FP32', 'SCATTER_FP32', 'WG_XN_ORDERED'), ('FWD_FP32', 'SCATTER_FP32', 'WG_XN_ORDERED'),
                         ('FWD_FP32', 'GATHER_MM', 'WG_XN_ORDERED'), ('FWD_FP32', 'SCATTER_FP32', 'WG_XN_ORDERED'),
                         ('FWD_FP32', 'GATHER_GROUPED', 'WG_FP32_ORDERED')),
    # bf16x6: 1 x 28 x 6144 = 172032 > 8 x 24 x 49 x 16 = 150528; bf16x3: 114688 fits
    'k7_dil2': _routes(('FWD_FP32', 'SCATTER_FP32', 'WG_XN_ORDERED'), ('FWD_FP32', 'SCATTER_FP32', 'WG_XN_ORDERED'),
                       ('FWD_FP32', 'GATHER_MM', 'WG_XN_ORDERED'), ('FWD_FP32', 'SCATTER_FP32', 'WG_XN_ORDERED'),
                       ('FWD_FP32', 'GATHER_GROUPED', 'WG_FP32_ORDERED')),
    'k8_bound': _routes(('FWD_FP32', 'GATHER_MM', 'WG_XN_ORDERED'), ('FWD_FP32', 'SCATTER_FP32', 'WG_XN_ORDERED'),
                        ('FWD_FP32', 'GATHER_MM', 'WG_XN_ORDERED'), ('FWD_FP32', 'SCATTER_FP32', 'WG_XN_ORDERED'),
                        ('FWD_FP32', 'GATHER_GROUPED', 'WG_FP32_ORDERED')),
    # forward: the 64-wide tile (16896 + 131072 = 147968; the 256-wide one would need 173312)
    'k4_dg4_bound': _routes(('FWD_FP32', 'GATHER_MM', 'WG_XN_ORDERED'), ('FWD_FP32', 'SCATTER_FP32', 'WG_XN_ORDERED'),
                            ('FWD_FP32', 'GATHER_MM', 'WG_XN_ORDERED'), ('FWD_FP32', 'SCATTER_FP32', 'WG_XN_ORDERED'),
                            ('FWD_FP32', 'GATHER_GROUPED', 'WG_FP32_ORDERED')),
}

# (case, kernel choice, pass) -> what lsn_last_error names.  A call outside this table is served; a call in it returns
# LSN_ERR_UNSUPPORTED in front of its first launch and leaves every buffer as it was.
EXPECTED_REFUSALS = {
    # SCATTER_FP32 at KD = 64, Co / groups = 32: RED = 64, 128 x 64 + 2816 x 64 = 188416 > 163840
    ('k8_bound', 'x6_first_gemms', 'bwd'): 'LDS',
    ('k8_bound', 'x3_atomic_fallbacks', 'bwd'): 'LDS',
    # SCATTER_FP32 at KD = 64, Co / groups = 128: RED = 256 needs 32768 + 180224 = 212992, RED = 64 the same 188416 > 163840
    ('k4_dg4_bound', 'x6_first_gemms', 'bwd'): 'LDS',
    ('k4_dg4_bound', 'x3_atomic_fallbacks', 'bwd'): 'LDS',
}
# KD = 75 > 64: check_shape, both passes, every choice ("kh*kw*deformable_groups = 75 > 64 is not supported")
for _choice in _SPLIT_CHOICES + ('math_fp32',):
    for _pass in ('fwd', 'bwd'):
        EXPECTED_REFUSALS[('k5_dg3_over', _choice, _pass)] = '> 64'
