"""LSHead's point decoding (ops/point_decode.py) with the library's kernels against the torch statements
(point_decode.NATIVE_POINTS off), on one GPU.

default        the head of the benchmark model (LSNet R-50 bbox, FPN maps of a 2 x 800 x 1344 batch) forward + backward on its
               own, then the whole training step, each with the switch off and on: device events around a loop of at least
               0.5 s, three alternating readings each way (profiles/native_points_step.txt)
--steps N      N training steps with the switch as LSNET_NATIVE_POINTS sets it and nothing else: run it under
               `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_points.py --steps 10` once each way
               for the launch counts (profiles/native_points_kernel_stats.txt)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import build_step  # noqa: E402
from lsnet_amd import _lib  # noqa: E402
from lsnet_amd.data import synthetic_batch  # noqa: E402
from lsnet_amd.model_zoo import build_lsnet  # noqa: E402
from lsnet_amd.ops import point_decode as point_ops  # noqa: E402
from lsnet_amd.parallel import DataParallelModel  # noqa: E402

DEV = torch.device('cuda:0')
CL = torch.channels_last


def timed(fn, min_s=0.5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    n = 5
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
            point_ops.NATIVE_POINTS = on
            rows.append((on, timed(fn)))
    point_ops.NATIVE_POINTS = True
    off = sorted(t for on, t in rows if not on)
    on_ = sorted(t for on, t in rows if on)
    print(f'{name}: torch statements {off[1]:.4f} ms (min {off[0]:.4f}, max {off[2]:.4f}); native {on_[1]:.4f} ms '
          f'(min {on_[0]:.4f}, max {on_[2]:.4f})', flush=True)


def model_and_step():
    _lib.set_math_mode('bf16x6')
    torch.manual_seed(0)
    model, cfg = build_lsnet('bbox', 'r50')
    model = DataParallelModel(model.to(DEV).to(memory_format=CL).train())
    step, _ = build_step(model, cfg)
    data = synthetic_batch('bbox', 2, 800, 1344, seed=1234, device=DEV, channels_last=True)
    return model, step, data


def modules():
    model, step, data = model_and_step()
    head = model.module.bbox_head if hasattr(model, 'module') else model.bbox_head
    g = torch.Generator().manual_seed(3)
    feats = [torch.randn(2, 256, -(-800 // s), -(-1344 // s), generator=g).to(DEV).contiguous(memory_format=CL).requires_grad_()
             for s in (8, 16, 32, 64, 128)]
    params = [p for p in head.parameters() if p.requires_grad]

    def head_fwd_bwd():
        outs = [t for lst in head(feats) for t in lst if t is not None]
        torch.autograd.grad(outs, feats + params, [torch.ones_like(t) for t in outs], allow_unused=True)
    pair('LSHead (bbox, 256 channels, 2 x 800 x 1344) forward + backward', head_fwd_bwd)
    pair('training step, LSNet R-50 bbox, 2 x 800 x 1344', lambda: step(data))


def steps(n):
    _, step, data = model_and_step()
    for _ in range(n):
        step(data)
    torch.cuda.synchronize()
    print(f'{n} steps, NATIVE_POINTS = {point_ops.NATIVE_POINTS}', flush=True)


if __name__ == '__main__':
    steps(int(sys.argv[sys.argv.index('--steps') + 1])) if '--steps' in sys.argv else modules()
