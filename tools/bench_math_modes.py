"""The benchmark step (bench.py: LSNet R-50 bbox, 2 x 3x800x1344, one GPU) in the math modes 'bf16x6', 'bf16x3' and 'bf16',
alternated in ONE process for several rounds so that every mode sees the same box, clocks and neighbours:

    python tools/bench_math_modes.py [--rounds 5] [--steps 10] [--warmup 3] [--modes bf16x6,bf16x3,bf16]

Per mode: median and minimum ms / step and img / s over the rounds, then the per-family kernel time of one step from the
library's event log (lsn_prof_*, as bench.py --full's survey).  Reuses bench.build_step / bench.timed_steps; one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
argv, sys.argv = sys.argv[1:], sys.argv[:1]   # bench.py parses its own arguments at import time
import bench  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--survey-steps', type=int, default=3)
    ap.add_argument('--modes', default='bf16x6,bf16x3,bf16')
    args = ap.parse_args(argv)
    from lsnet_amd import _lib
    from lsnet_amd.data import synthetic_batch
    from lsnet_amd.model_zoo import build_lsnet
    from lsnet_amd.parallel import DataParallelModel
    assert torch.cuda.is_available(), 'bench_math_modes.py measures on the GPU'
    dev = torch.device('cuda:0')
    modes = args.modes.split(',')
    torch.manual_seed(0)
    model, cfg = build_lsnet('bbox', 'r50')
    model = DataParallelModel(model.to(dev).to(memory_format=torch.channels_last).train())
    step, _ = bench.build_step(model, cfg)
    data = synthetic_batch('bbox', 2, 800, 1344, seed=1234, device=dev, channels_last=True)
    before = _lib.get_math_mode()
    ms = {m: [] for m in modes}
    kernels = {}
    try:
        for m in modes:   # warm every mode's shapes and images once before the timed rounds
            _lib.set_math_mode(m)
            bench.timed_steps(step, data, 1, args.warmup)
        for _ in range(args.rounds):
            for m in modes:
                _lib.set_math_mode(m)
                ms[m].append(1e3 * bench.timed_steps(step, data, args.steps, 1))
        timer = bench.KernelTimer()
        for m in modes:
            _lib.set_math_mode(m)
            step(data)
            timer.start()
            for _ in range(args.survey_steps):
                step(data)
            ks = timer.stop()
            kernels[m] = {f: dict(ms_per_step=round(v['total_ms'] / args.survey_steps, 3),
                                  launches_per_step=v['launches'] // args.survey_steps, tflops=round(v['tflops'], 1))
                          for f, v in sorted(ks.items(), key=lambda kv: -kv[1]['total_ms'])}
    finally:
        _lib.set_math_mode(before)
    img = data['img'].shape[0]
    res = {m: dict(ms_per_step_median=round(statistics.median(v), 2), ms_per_step_min=round(min(v), 2),
                   img_per_s_median=round(img * 1e3 / statistics.median(v), 1), img_per_s_max=round(img * 1e3 / min(v), 1),
                   rounds_ms=[round(t, 2) for t in v], kernels=kernels[m]) for m, v in ms.items()}
    print(json.dumps(dict(workload='R-50 bbox train step, 2 x 3x800x1344, 1 GPU', device=torch.cuda.get_device_name(0),
                          rounds=args.rounds, steps_per_round=args.steps, modes=res)))


if __name__ == '__main__':
    main()
