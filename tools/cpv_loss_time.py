"""The loss section of LSNet-CPV (LSCPVHead.loss + the backward of the sum of its losses) with the corner-verification targets
and losses as kernels of the library against the torch statements (LSNET_NATIVE_CPV=0), on one GPU, on STORED head outputs:
the `bbox_cpv` model of model_zoo (R-50-FPN, random-init weights) runs once on synthetic_batch('bbox_cpv', 2, 800, 1344) and
the loss section alone is measured on what its head returned, the tensors in the head's own layout.

Every reading runs in a fresh child process (the switch is read at import); the two arms alternate; the parent prints the
median and the spread of
  device ms    device events around a loop of at least 0.5 s after warm-up
  enqueue ms   host clock from the first statement of an iteration to the return of its last launch, no synchronise inside the
               loop (when this exceeds the device time the section is bound by the host)
  launches     device kernel rows of one iteration under torch.profiler (a run of its own, after the timed loops)

  python tools/cpv_loss_time.py [--readings N]          -> profiles/native_cpv_loss.txt"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, H, W = 2, 800, 1344


def child():
    import torch
    from torch.profiler import ProfilerActivity, profile

    from lsnet_amd.data import synthetic_batch
    from lsnet_amd.model_zoo import build_lsnet
    from lsnet_amd.ops import cpv_loss
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model, _ = build_lsnet('bbox_cpv', 'r50')
    model = model.to(dev).to(memory_format=torch.channels_last).train()
    data = synthetic_batch('bbox_cpv', B, H, W, seed=1234, device=dev)
    with torch.no_grad():
        outs = model.bbox_head(model.extract_feat(data['img']))
    head = model.bbox_head
    leaves = [[t.detach().requires_grad_() for t in lv] for lv in outs]
    del model, outs

    def section():
        losses = head.loss(*leaves, data['gt_bboxes'], data['gt_extremes'], data['gt_sem_map'], data['gt_sem_weights'],
                           data['gt_labels'], data['img_metas'])
        total = sum(sum(v) if isinstance(v, (list, tuple)) else v for v in losses.values())
        total.backward()
        return total

    for _ in range(5):
        section()
    torch.cuda.synchronize()
    n = 10
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for _ in range(n):
            section()
        b.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 500:
            break
        n = int(n * max(2.0, 500 / max(ms, 1e-3) * 1.2))
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        total = section()
        torch.cuda.synchronize()
    launches = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    print(json.dumps(dict(native=cpv_loss.NATIVE_CPV, device_ms=ms / n, enqueue_ms=(t1 - t0) * 1000 / n, launches=launches,
                          iterations=n, loss=float(total))), flush=True)


def main():
    readings = int(sys.argv[sys.argv.index('--readings') + 1]) if '--readings' in sys.argv else 3
    rows = []
    for r in range(readings):
        for native in (False, True):
            env = dict(os.environ, LSNET_NATIVE_CPV='1' if native else '0')
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=env, cwd=ROOT, check=True,
                                 stdout=subprocess.PIPE, text=True).stdout
            row = json.loads([l for l in out.splitlines() if l.startswith('{')][-1])
            assert row['native'] == native
            rows.append(row)
            print(f'reading {r} {"native" if native else "torch statements"}: {row}', flush=True)
    print(f'\nLSCPVHead.loss + backward on stored head outputs, {B} x 3x{H}x{W}, R-50-FPN bbox_cpv, {readings} alternating readings '
          f'per arm, each in a fresh process: median (min .. max)')
    for native, name in ((False, 'torch statements (LSNET_NATIVE_CPV=0)'), (True, 'native')):
        line = f'  {name}:'
        for key, unit in (('device_ms', ' ms device'), ('enqueue_ms', ' ms host enqueue'), ('launches', ' launches')):
            v = sorted(row[key] for row in rows if row['native'] == native)
            fmt = '{:.0f}' if key == 'launches' else '{:.3f}'
            line += f' {fmt.format(v[len(v) // 2])} ({fmt.format(v[0])} .. {fmt.format(v[-1])}){unit};'
        print(line + f' loss {[row["loss"] for row in rows if row["native"] == native][0]:.6f}')


if __name__ == '__main__':
    child() if '--child' in sys.argv else main()
