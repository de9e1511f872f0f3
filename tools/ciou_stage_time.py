"""One regression stage of LSHead.loss_levels for the segm (polygon, nv = 36, 9 subsets) and the pose (keypoint, nv = 17) task,
forward + backward, on STORED inputs at the workload's size: n = 44,800 rows (2 images x 22,400 points of a 800 x 1344 image,
the strides distributed as the five levels are), about 0.2 % of the rows carrying an object.

  arm A  LSNET_CIOU_STAGE=0: the torch statements of loss_levels (pred * stride, _gt_reg, the divisions by norm) + the fused
         rows behind CrossIOULoss (lsn_cross_iou_rows_*): the path before the stage kernels
  arm B  the stage call (ops.cross_iou.cross_iou_stage_rows, lsn_cross_iou_stage_*)

Every reading runs in a fresh child process; the two arms alternate; the parent prints the median and the spread of
  device ms    device events around a loop of at least 0.5 s after warm-up
  enqueue ms   host clock from the first statement of an iteration to the return of its last launch, no synchronise inside
  launches     device kernel rows of one iteration under torch.profiler (a run of its own, after the timed loops)
then the time of the stage kernels themselves from a `rocprofv3 --kernel-trace --stats` run of its own beside their
bytes-over-bandwidth floor, and (--whole-step N) N alternating readings of tools/config_steps.py segm x101-dcn each way.

  python tools/ciou_stage_time.py [--readings N] [--whole-step N]          -> profiles/native_ciou_stage.txt"""
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'native_ciou_stage.txt')
LINES = []


def say(line=''):
    print(line, flush=True)
    LINES.append(line)


B, LEVELS, STRIDES = 2, [100 * 168, 50 * 84, 25 * 42, 13 * 21, 7 * 11], [8., 16., 32., 64., 128.]
BASE_SCALE, OBJECT_SHARE, PEAK = 4.0, 0.002, 6.3e12           # achievable HBM bandwidth of the MI355X in B/s
KINDS = {'polygon': dict(nv=36, sub=9), 'keypoint': dict(nv=17, sub=9)}
# bytes per row: raw prediction, points, anchor3, box or visibilities, weight; backward adds the upstream gradient and grad_raw
ROW_BYTES = {'polygon': (148 * 4 + 74 * 4 + 12 + 16 + 4, 4 + 148 * 4), 'keypoint': (72 * 4 + 36 * 4 + 12 + 17 * 4 + 4, 4 + 72 * 4)}


def stored_inputs(kind, dev):
    import torch
    nv = KINDS[kind]['nv']
    g = torch.Generator().manual_seed(7)
    n = B * sum(LEVELS)
    stride = torch.cat([torch.full((c,), s) for c, s in zip(LEVELS, STRIDES)]).repeat(B)[:, None]
    anchor = torch.cat([torch.floor(torch.rand(n, 2, generator=g) * 100) * stride, stride], 1)
    raw = torch.rand(n, 4 * (nv + 1), generator=g) * 2 + 0.01
    obj = torch.rand(n, generator=g) < OBJECT_SHARE
    pts = anchor[:, :2].repeat(1, nv + 1) + torch.randn(n, 2 * (nv + 1), generator=g) * stride * 2
    xs, ys = pts[:, 0:2 * nv:2], pts[:, 1:2 * nv:2]
    box = torch.stack([xs.min(1)[0], ys.min(1)[0], xs.max(1)[0], ys.max(1)[0]], 1)
    pts, box = pts * obj[:, None], box * obj[:, None]
    vs = (torch.rand(n, nv, generator=g) > 0.3).float() * 2
    bw = obj.float()[:, None].expand(-1, 4).contiguous()        # the head's bbox_weights
    return dict(raw=raw.to(dev).requires_grad_(), gt_pts=pts.to(dev), anchor=anchor.to(dev), box=box.to(dev), vs=vs.to(dev),
                bw=bw.to(dev), stride=stride.to(dev), norm=(BASE_SCALE * stride).to(dev), n_obj=int(obj.sum()))


def make_section(kind, c):
    """one stage the way LSHead.loss_levels runs it, + the backward of the sum of its rows"""
    from lsnet_amd.models.dense_heads.ls_head import LSHead
    from lsnet_amd.models.losses import CrossIOULoss
    from lsnet_amd.ops import cross_iou as fused
    loss_fn = CrossIOULoss(loss_type=kind, loss_weight=1.0, stride=KINDS[kind]['sub'])
    raw, gt_pts, anchor, bbox_gt, bw, stride, norm = c['raw'], c['gt_pts'], c['anchor'], c['box'], c['bw'], c['stride'], c['norm']
    kw = {} if kind == 'polygon' else dict(bbox_gt=None, vs=c['vs'])
    width = raw.shape[1]

    def section():
        raw.grad = None
        if fused.stage_enabled():
            rows = loss_fn.loss_weight * fused.cross_iou_stage_rows(kind, raw, gt_pts, anchor, bbox_gt, kw.get('vs'), bw[:, 0],
                                                                    BASE_SCALE, loss_fn.alpha, loss_fn.eps, loss_fn.stride)
        else:
            kw_ = dict(bbox_gt=bbox_gt / norm) if kind == 'polygon' else kw
            weights = bw[:, :1].expand(-1, width)
            pred = raw * stride
            gt_reg, active = LSHead._gt_reg(gt_pts, anchor, weights)
            rows = loss_fn(pred / norm, gt_reg / norm, weights, reduction_override='none', anchor_pts=anchor[:, :-1] / norm,
                           pos_inds=active, **kw_)
        total = rows.sum()
        total.backward()
        return total
    return section


def child(kind):
    import torch
    from torch.profiler import ProfilerActivity, profile

    from lsnet_amd.ops import cross_iou as fused
    dev = torch.device('cuda:0')
    c = stored_inputs(kind, dev)
    section = make_section(kind, c)
    for _ in range(5):
        section()
    torch.cuda.synchronize()
    if '--trace' in sys.argv:                                    # under rocprofv3: a few iterations, nothing else
        for _ in range(20):
            section()
        torch.cuda.synchronize()
        return
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
    print(json.dumps(dict(kind=kind, stage=fused.stage_enabled(), device_ms=ms / n, enqueue_ms=(t1 - t0) * 1000 / n,
                          launches=launches, iterations=n, loss=float(total), grad=float(c['raw'].grad.abs().sum()),
                          rows=c['raw'].shape[0], objects=c['n_obj'])), flush=True)


def spread(values, fmt='{:.3f}'):
    v = sorted(values)
    return f'{fmt.format(statistics.median(v))} ({fmt.format(v[0])} .. {fmt.format(v[-1])})'


def kernel_times():
    """-> {(kind, 'forward' | 'backward'): [us]} of lsn::cross_iou_stage_kernel from a kernel trace of arm B"""
    prof = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    out = {}
    for kind in KINDS:
        d = tempfile.mkdtemp(prefix='ciou_stage_')
        try:
            run = subprocess.run([prof, '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 't', '--',
                                  sys.executable, os.path.abspath(__file__), '--child', kind, '--trace'],
                                 env=dict(os.environ, LSNET_CIOU_STAGE='1'), cwd=ROOT, stdout=subprocess.PIPE,
                                 stderr=subprocess.STDOUT, text=True)
            if run.returncode:
                raise RuntimeError(f'rocprofv3 ended with {run.returncode}:\n{run.stdout[-2000:]}')
            files = glob.glob(d + '/**/*kernel_trace.csv', recursive=True)
            for r in csv.DictReader(open(files[0])):
                m = re.search(r'cross_iou_stage_kernel<(true|false)>', r['Kernel_Name'])
                if m:
                    out.setdefault((kind, 'backward' if m.group(1) == 'true' else 'forward'), []).append(
                        (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
        finally:
            shutil.rmtree(d, ignore_errors=True)
    return out


def whole_step(readings):
    rows = {'0': [], '1': []}
    for r in range(readings):
        for arm in ('0', '1'):
            out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'config_steps.py'), 'segm', 'x101-dcn', '10'],
                                 env=dict(os.environ, LSNET_CIOU_STAGE=arm), cwd=ROOT, check=True, stdout=subprocess.PIPE,
                                 text=True).stdout
            ms = float(re.search(r'([\d.]+) ms/step untraced-in-process', out).group(1))
            rows[arm].append(ms)
            say(f'whole step reading {r} LSNET_CIOU_STAGE={arm}: {ms:.2f} ms/step')
    say(f'\nconfig 4 (tools/config_steps.py segm x101-dcn 10: 2 x 3x800x1344, 10 steps after 3 of warm-up), {readings} alternating '
          f'readings per arm, each in a fresh process: median (min .. max)')
    for arm, name in (('0', 'A  LSNET_CIOU_STAGE=0'), ('1', 'B  stage kernels    ')):
        say(f'  {name}: {spread(rows[arm], "{:.2f}")} ms/step')


def main():
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default      # noqa: E731
    readings, steps = arg('--readings', 3), arg('--whole-step', 0)
    rows = []
    for r in range(readings):
        for kind in KINDS:
            for arm in ('0', '1'):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', kind], cwd=ROOT, check=True,
                                     env=dict(os.environ, LSNET_CIOU_STAGE=arm, LSNET_FUSED_CIOU='1'), stdout=subprocess.PIPE,
                                     text=True).stdout
                row = json.loads([ln for ln in out.splitlines() if ln.startswith('{')][-1])
                assert row['stage'] == (arm == '1')
                rows.append(row)
                say(f'reading {r} {kind} {"B stage call" if row["stage"] else "A statements + rows"}: {row}')
    say(f'\nOne regression stage, forward + backward of the sum of its rows, on stored inputs: {rows[0]["rows"]} rows, '
          f'{readings} alternating readings per arm, each in a fresh process: median (min .. max)')
    med = {}
    for kind, cfg in KINDS.items():
        objects = [r['objects'] for r in rows if r['kind'] == kind][0]
        say(f'  {kind} (nv {cfg["nv"]}' + (f', {cfg["sub"]} subsets' if kind == 'polygon' else '') + f', {objects} rows with an object)')
        for stage, name in ((False, 'A  statements + cross_iou_rows (LSNET_CIOU_STAGE=0)'), (True, 'B  stage call')):
            sel = [r for r in rows if r['kind'] == kind and r['stage'] == stage]
            med[kind, stage] = statistics.median(r['device_ms'] for r in sel)
            say(f'    {name}: {spread(r["device_ms"] for r in sel)} ms device; {spread(r["enqueue_ms"] for r in sel)} ms host enqueue; '
                  f'{spread((r["launches"] for r in sel), "{:.0f}")} launches; loss {sel[0]["loss"]:.6f}  sum |grad| {sel[0]["grad"]:.6f}')
        faster = med[kind, True] < med[kind, False]
        say(f'    -> arm B is {"FASTER" if faster else "NOT faster"}: {med[kind, False] / med[kind, True]:.2f} x')
    say('\nThe stage kernels alone (rocprofv3 --kernel-trace --stats, a run of its own, 25 launches each) beside the floor bytes / '
          f'{PEAK / 1e12:.1f} TB/s of their shapes:')
    n = rows[0]['rows']
    for (kind, way), us in sorted(kernel_times().items()):
        fwd, extra = ROW_BYTES[kind]
        nbytes = n * (fwd + 4 if way == 'forward' else fwd + extra)
        floor = nbytes / PEAK * 1e6
        say(f'  {kind:8s} {way:8s}: {spread(us, "{:.1f}")} us over {len(us)} launches; {nbytes / 1e6:.1f} MB -> floor {floor:.1f} us; '
              f'{100 * floor / statistics.median(us):.0f} % of the achievable bandwidth')
    say('\nRegisters and LDS of the stage kernels (tools/kernel_resources.sh loss.hip cross_iou_stage; the LDS is dynamic: a tile of '
        '64 rows at odd pitches + 4 values per row):')
    res = subprocess.run(['bash', os.path.join(ROOT, 'tools', 'kernel_resources.sh'), 'loss.hip', 'cross_iou_stage'],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    for ln in res.splitlines():
        if 'cross_iou_stage_kernel' in ln:
            say('  ' + ' '.join(ln.split()))
    for kind, cfg in KINDS.items():
        m = 4 * (cfg['nv'] + 1)
        lds = 64 * 4 * ((m + 1) + (m // 2 + 1) + ((cfg['nv'] | 1) if kind == 'keypoint' else 0) + 4)
        say(f'  {kind}: {lds} B of LDS per workgroup of one wave -> {160 * 1024 // lds} workgroups per CU, '
            f'{-(-n // 64)} tiles on {256 * (160 * 1024 // lds)} slots')
    if steps:
        say()
        whole_step(steps)
    with open(OUT, 'w') as fh:
        fh.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    child(sys.argv[sys.argv.index('--child') + 1]) if '--child' in sys.argv else main()
