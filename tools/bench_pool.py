"""The pooling family (ops/pool.py, ops/corner_pool.py) with the library's kernels against the framework's statements
(pool.NATIVE_POOL off), on one GPU.

default   module times: forward + backward of Res2Net's strided Bottle2neck blocks, of a TLPool block and of single ops at the
          models' sizes, device events around a loop of at least 0.5 s, three alternating readings each way
          (profiles/native_pool_step.txt)
--trace   ten iterations of each op's forward + backward each way and nothing else: run it under
          `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_pool.py --trace` for kernel times
          (profiles/native_pool_kernel_stats.txt)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from lsnet_amd.models import build_backbone  # noqa: E402
from lsnet_amd.ops import corner_pool as cp  # noqa: E402
from lsnet_amd.ops import pool  # noqa: E402
from tests import golden_util as gu  # noqa: E402

DEV = torch.device('cuda:0')
CL = torch.channels_last


def timed(fn, min_s=0.5):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    n = 10
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= min_s * 1000:
            return ms / n
        n = int(n * max(2.0, min_s * 1000 / max(ms, 1e-3) * 1.2))


def pair(name, fn):
    rows = []
    for r in range(3):
        for on in (False, True):
            pool.NATIVE_POOL = on
            rows.append((on, timed(fn)))
    pool.NATIVE_POOL = True
    off = sorted(t for on, t in rows if not on)
    on_ = sorted(t for on, t in rows if on)
    print(f'{name}: framework statements {off[1]:.4f} ms (min {off[0]:.4f}, max {off[2]:.4f}); native {on_[1]:.4f} ms '
          f'(min {on_[0]:.4f}, max {on_[2]:.4f})', flush=True)


def fwd_bwd(module, x, params):
    go = torch.randn_like(module(x))

    def run():
        torch.autograd.grad(module(x), [x] + params, go)
    return run


def t(*shape, relu=False):
    x = torch.randn(*shape, device=DEV)
    return (torch.relu(x) if relu else x).contiguous(memory_format=CL).requires_grad_()


def modules():
    torch.manual_seed(0)
    bb = build_backbone(dict(type='Res2Net', depth=50, scales=4, base_width=26, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=-1,
                             norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True))
    gu.fill_params(bb, seed=8)
    for li, (c, hw) in (('layer2', (256, (200, 336))), ('layer3', (512, (100, 168))), ('layer4', (1024, (50, 84)))):
        block = getattr(bb, li)[0].to(DEV).train().to(memory_format=CL)
        for m in block.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.eval()
        x = torch.randn(2, c, *hw, device=DEV).contiguous(memory_format=CL).requires_grad_()
        pair(f'Bottle2neck stage block {li}[0], input 2x{c}x{hw[0]}x{hw[1]}, forward + backward',
             fwd_bwd(block, x, [p for p in block.parameters() if p.requires_grad]))
        del block, x
    for hw in ((100, 168), (50, 84), (25, 42)):
        block = cp.TLPool(64, norm_cfg=dict(type='GN', num_groups=32, requires_grad=True), corner_dim=64)
        gu.fill_params(block, seed=9)
        block = block.to(DEV).train().to(memory_format=CL)
        x = torch.randn(2, 64, *hw, device=DEV).contiguous(memory_format=CL).requires_grad_()
        pair(f'TLPool (CornerPoolPack, 64 corner channels), input 2x64x{hw[0]}x{hw[1]}, forward + backward',
             fwd_bwd(block, x, list(block.parameters())))
        a = torch.relu(torch.randn(2, 64, *hw, device=DEV)).contiguous(memory_format=CL).requires_grad_()
        b = torch.relu(torch.randn(2, 64, *hw, device=DEV)).contiguous(memory_format=CL).requires_grad_()
        go = torch.randn_like(a)
        pair(f'pool_top(a) + pool_left(b) alone, 2x64x{hw[0]}x{hw[1]}, forward + backward',
             lambda: torch.autograd.grad(cp.corner_pool_sum(a, 'top', b, 'left'), [a, b], go))
    x = torch.randn(2, 64, 400, 672, device=DEV).contiguous(memory_format=CL).requires_grad_()
    go = torch.randn(2, 64, 200, 336, device=DEV).contiguous(memory_format=CL)
    pair('stem max pool 3/2/1, 2x64x400x672, forward + backward', lambda: torch.autograd.grad(pool.max_pool2d(x, 3, 2, 1), x, go))
    top = torch.randn(2, 256, 50, 84, device=DEV).contiguous(memory_format=CL).requires_grad_()
    lat = torch.randn(2, 256, 100, 168, device=DEV).contiguous(memory_format=CL).requires_grad_()
    go = torch.randn_like(lat)
    pair('upsample-add 50x84 -> 100x168, 2x256, forward + backward', lambda: torch.autograd.grad(pool.upsample_add(top, lat), [top, lat], go))


def trace():
    a, b = t(2, 64, 100, 168, relu=True), t(2, 64, 100, 168, relu=True)
    gc_ = torch.randn(2, 64, 100, 168, device=DEV).contiguous(memory_format=CL)
    x = t(2, 64, 400, 672)
    gm = torch.randn(2, 64, 200, 336, device=DEV).contiguous(memory_format=CL)
    top, lat = t(2, 256, 50, 84), t(2, 256, 100, 168)
    gu_ = torch.randn(2, 256, 100, 168, device=DEV).contiguous(memory_format=CL)
    wide = t(2, 416, 100, 168)
    ga = torch.randn(2, 104, 50, 84, device=DEV).contiguous(memory_format=CL)
    for on in (False, True):
        pool.NATIVE_POOL = on
        for _ in range(10):
            torch.autograd.grad(cp.corner_pool_sum(a, 'top', b, 'left'), [a, b], gc_)
            torch.autograd.grad(cp.corner_pool_sum(a, 'bottom', b, 'right'), [a, b], gc_)
            torch.autograd.grad(pool.max_pool2d(x, 3, 2, 1), x, gm)
            torch.autograd.grad(pool.upsample_add(top, lat), [top, lat], gu_)
            torch.autograd.grad(pool.avg_pool2d(wide[:, 312:], 3, 2, 1), wide, ga)
        torch.cuda.synchronize()


if __name__ == '__main__':
    trace() if '--trace' in sys.argv else modules()
