"""What does a ragged batch cost the training step?  The R-50 bbox model and the batch of bench.py (2 x 3 x 800 x 1344), once
with one `pad_shape` for both images (every grid cell valid) and once with the second image 800 x 1216 inside the padded
batch, its gts inside that -- what a data loader that pads a batch to its largest member feeds.  Per batch: ms per step
(forward_train + backward + clip + SGD, device events around a synchronised window), the synchronising calls of one step
(torch.cuda.set_sync_debug_mode('warn'), as tools/cpu_lead.py counts them) and the launches of the library's instrumented
kernel families in one step (lsn_prof_*).  Uses only interfaces that predate the masked assignment calls, so the same file
measures an older tree: copy it there and run both alternately (profiles/native_ragged_assign.txt).
    python tools/ragged_targets.py [steps] [tag]"""
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
tag = sys.argv[2] if len(sys.argv) > 2 else 'tree'
sys.argv = sys.argv[:1]
import bench  # noqa: E402
from lsnet_amd import _lib  # noqa: E402
from lsnet_amd.data import synthetic_batch  # noqa: E402
from lsnet_amd.model_zoo import build_lsnet  # noqa: E402
from lsnet_amd.parallel import DataParallelModel  # noqa: E402

H, W, W_SMALL = 800, 1344, 1216
dev = torch.device('cuda:0')
torch.manual_seed(0)
model, cfg = build_lsnet('bbox', 'r50')
model = DataParallelModel(model.to(dev).to(memory_format=torch.channels_last).train())
step, runner = bench.build_step(model, cfg)

full = synthetic_batch('bbox', 2, H, W, seed=1234, device=dev, channels_last=True)
small = synthetic_batch('bbox', 2, H, W_SMALL, seed=1234, device=dev, channels_last=True)
ragged = dict(full)
ragged['img_metas'] = [full['img_metas'][0], dict(full['img_metas'][1], pad_shape=(H, W_SMALL, 3), img_shape=(H, W_SMALL, 3))]
for k in ('gt_bboxes', 'gt_labels', 'gt_extremes'):
    ragged[k] = [full[k][0], small[k][1]]
del small


def measure(name, data):
    for _ in range(4):                      # warm the shape: constants of the geometry, workspaces, the allocator
        step(data)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        step(data)
        torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('default')
    sync = [x for x in w if 'synchroniz' in str(x.message).lower()]
    _lib.prof_enable(True)
    step(data)
    torch.cuda.synchronize()
    fam = _lib.prof_read()
    _lib.prof_enable(False)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        out = step(data)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    print(f'{tag} {name:9s} {ms:8.3f} ms/step over {steps} steps | synchronising calls in one step: {len(sync):3d} | '
          f'library launches in one step (instrumented families): {sum(f["launches"] for f in fam.values())} | '
          f'loss {float(out["loss"]):.6f}', flush=True)
    where = {}
    for x in sync:
        key = (os.path.relpath(x.filename, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), x.lineno)
        where[key] = where.get(key, 0) + 1
    for (f, line), n in sorted(where.items()):
        print(f'{tag} {name:9s}     {n} x {f}:{line}', flush=True)
    return ms


a = measure('all-valid', full)
b = measure('ragged', ragged)
print(f'{tag} ragged / all-valid = {b / a:.4f}', flush=True)
