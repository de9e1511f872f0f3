"""The detection decode (LSHead.get_bboxes: per-level top-k, vector decode, multi-class NMS) with the library's lsn_decode_batch
against the torch statements (ls_head.NATIVE_DECODE off), on one GPU, on STORED head outputs: LSNet R-50-FPN runs once on
4 images 3x800x1344 (random-init weights, as bench.py's inference leg) and get_bboxes alone is timed on what its head returned
-- the tensors in the head's own layout, views into its concatenated channels-last outputs.

  pose_kbox  C = 1; the classification bias is shifted by +2 as bench.py's infer_pose_bs4 does, so nearly every selected point
             passes score_thr = 0.05 (up to 3350 candidates per image: 3 x 1000 + 273 + 77 selected points)
  bbox       C = 80; the same shift on ONE class per point (a fixed random choice), which gives the same number of
             candidates per image -- the shift on all 80 classes would make 268 000, far from any trained detector
  bbox_cpv   the corner-verification head (LSCPVHead.get_bboxes, lsn_decode_cpv_batch), C = 80 with the shift of `bbox`; its
             corner heat-maps and offsets are what the random-init head returned (profiles/native_decode_cpv.txt)

default       device events around a loop of at least 0.5 s after warm-up, three alternating readings each way
              (profiles/native_decode_step.txt)
--way torch   only the torch statements (this is what runs on a tree that has no native decode); --way native: only the kernels
--readings N  N alternating readings each way instead of three
--task NAME   only that task (default: all three)
--trace       ten iterations each way and nothing else: run it under
              `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_decode.py --trace` for kernel times
              (profiles/native_decode_kernel_stats.txt)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from lsnet_amd.model_zoo import build_lsnet  # noqa: E402
from lsnet_amd.models.dense_heads import ls_head  # noqa: E402

DEV = torch.device('cuda:0')
B, H, W = 4, 800, 1344


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


def stored_outputs(task):
    """(head, its outputs for 4 random images, metas): the model is dropped, the outputs stay on the device."""
    torch.manual_seed(0)
    model, _ = build_lsnet(task, 'r50')
    model = model.to(DEV).to(memory_format=torch.channels_last).eval()
    img = torch.randn(B, 3, H, W, device=DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        outs = model.bbox_head(model.extract_feat(img))
        g = torch.Generator().manual_seed(1)
        for c in outs[0]:
            if c.shape[1] == 1:
                c.add_(2.0)
            else:
                pick = torch.randint(0, c.shape[1], (c.shape[0], 1, *c.shape[2:]), generator=g).to(DEV)
                c.scatter_add_(1, pick, torch.full(pick.shape, 2.0, device=DEV))
    metas = [dict(pad_shape=(H, W, 3), img_shape=(H, W, 3), scale_factor=1.0, ori_shape=(H, W, 3), flip=False)] * B
    head = model.bbox_head
    del model
    return head, outs, metas


def readings():
    return int(sys.argv[sys.argv.index('--readings') + 1]) if '--readings' in sys.argv else 3


def ways():
    if '--way' in sys.argv:
        return [sys.argv[sys.argv.index('--way') + 1] == 'native']
    return [False, True]


def main(trace):
    tasks = [sys.argv[sys.argv.index('--task') + 1]] if '--task' in sys.argv else ['pose_kbox', 'bbox', 'bbox_cpv']
    for task in tasks:
        head, outs, metas = stored_outputs(task)

        def run():
            with torch.no_grad():
                return head.get_bboxes(*outs, metas)
        rows = []
        for r in range(1 if trace else readings()):
            for on in ways():
                ls_head.NATIVE_DECODE = on
                if trace:
                    for _ in range(10):
                        run()
                    torch.cuda.synchronize()
                else:
                    rows.append((on, timed(run)))
        ls_head.NATIVE_DECODE = True
        if trace:
            continue
        dets = run()
        line = f'{task}: get_bboxes on {B} x 3x{H}x{W}, C = {outs[0][0].shape[1]}, detections {[int(d[0].shape[0]) for d in dets]}:'
        for on, name in ((False, 'torch statements'), (True, 'native')):
            t = sorted(v for o, v in rows if o == on)
            if t:
                line += f' {name} {t[len(t) // 2]:.4f} ms (min {t[0]:.4f}, max {t[-1]:.4f});'
        print(line, flush=True)


if __name__ == '__main__':
    main('--trace' in sys.argv)
