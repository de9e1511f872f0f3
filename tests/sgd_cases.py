"""Reference, storage layout and cases of the clip + SGD step tests (tests/test_fused_sgd_host.py, tests/test_fused_sgd_seams_gpu.py).

`reference_step` is the operator sequence the library's step replaces (clip_grad_norm_ + torch.optim.SGD.step(),
mmcv/runner/hooks/optimizer.py:8-28) in float64 on the CPU; the host test compares it with torch's own float64 path.

`Layout` places a list of shapes the way training does: the gradients are views into the buckets of a
`BucketedGradReducer` (world size 1, a small `bucket_mb`: several buckets, hence one arena), parameters and momentum
buffers are 16-byte-aligned views of one flat tensor each with slots rounded as the reducer rounds them.  Every float of
the three flat tensors that no view owns -- slot pads, arena gaps between buckets, guard bands -- holds SENTINEL: a store
past a tensor's end changes its bits, a load past it makes the norm infinite (SENTINEL ** 2 overflows fp32).

`run_case` drives four steps of a subject (`make_plan(optimizer, grad_clip)` -> an object with ok / still_valid() / step() /
stats, i.e. runner/fused_sgd.py: ClipSGD) with the schedule of tests/test_fused_sgd_gpu.py: the learning rate changes every
step and the gradients of step 2 are 100 x larger, so that clipping switches on and off.

Error measure (BOUND = 2e-6, the figure of tests/test_fused_sgd_gpu.py): a tensor's error against float64 is divided by
the largest OPERAND of its update -- max |p|, max |buf|, max |g| before the step, finite values only -- not by the result:
a one-element tensor's result cancels (torch's own fp32 path is 4.6e-5 of the result there, 1.4e-7 of the operands).
Non-finite entries have to agree exactly (NaN with NaN, inf with the same inf)."""
import copy
import functools

import torch

from lsnet_amd.parallel.reducer import BucketedGradReducer

SENTINEL = 1e30
GUARD = 64                  # floats of SENTINEL in front of the first and behind the last view of a flat tensor
BOUND = 2e-6
STEPS = 4

BASE = ((0.02, 0.9, 1e-4),)                       # (lr, momentum, weight_decay) of the existing test
GROUPS3 = ((0.02, 0.9, 1e-4), (0.05, 0.8, 0.0), (0.01, 0.95, 5e-4))
GROUPS8 = GROUPS3 + ((0.03, 0.5, 1e-3), (0.04, 0.99, 2e-4), (0.015, 0.7, 1e-2), (0.025, 0.85, 3e-5), (0.06, 0.6, 7e-4))

# float4 body and scalar tail meet at numel % 4 and at multiples of the 4096-float chunk
SEAMS = ((1,), (2,), (3,), (4,), (5,), (27,), (4095,), (4096,), (4097,), (8191,), (8192,), (8193,),
         (27, 256, 3, 3), (5, 3, 1, 1), (64, 32, 3, 3))
# 2 + 2124 + 2 + 1 + 3 + 1 + 1 + 1 + 2 + 1 = 2138 chunks on 2048 workgroups: chunk 2048 lies inside the large tensor, tensor
# boundaries at chunks 2 and 2126; workgroups 0 and 1 meet another tensor on their second trip, 78 .. 89 the small ones
BIG = ((5000,), (2123 * 4096 + 77,), (4097,), (27,), (8193,), (1,), (5, 3, 1, 1), (4095,), (6001,), (3,))
# 11 tensors: dealt round-robin to 3 or 8 groups; index 4 (group 1 of 3: weight_decay 0) ends in a one-float tail
MIXED = ((7,), (64, 32, 3, 3), (2,), (33,), (4097,), (1000, 13), (5, 3, 1, 1), (8193,), (27,), (16, 8, 3, 3), (1,))
TABLE_SIZES = (1, 2, 3, 255, 256, 257)


def table_shapes(n):
    g = torch.Generator().manual_seed(4000 + n)
    return tuple((int(v),) for v in torch.randint(1, 6001, (n,), generator=g))


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def reference_step(params, grads, bufs, groups, group_of, max_norm):
    """One clip + SGD step on float64 CPU tensors.  `bufs[i]` is None on a tensor's first step, `groups[k]` =
    (lr, momentum, weight_decay), `group_of[i]` the group of tensor i, `max_norm` None: no clipping.
    -> (new params, new buffers, the gradients as the step leaves them, norm, coefficient)."""
    norm = torch.sqrt(sum((g * g).sum() for g in grads))
    if max_norm is None:
        coef = torch.ones((), dtype=torch.float64)
    else:
        coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)        # min(1, .) that keeps a NaN, as clip_grad_norm_ does
    new_p, new_b, new_g = [], [], []
    for p, g, b, k in zip(params, grads, bufs, group_of):
        lr, m, wd = groups[k]
        gs = g * coef
        d = gs if wd == 0 else gs + wd * p                           # torch adds nothing at weight_decay 0 (0 * inf is NaN)
        nb = d if b is None else m * b + d
        new_p.append(p - lr * nb), new_b.append(nb), new_g.append(gs)
    return new_p, new_b, new_g, norm, coef


def group_lists(tensors, n_groups):
    """round-robin: neighbours in memory differ in group"""
    return [[t for i, t in enumerate(tensors) if i % n_groups == k] for k in range(n_groups)]


def make_sgd(tensors, groups, **kw):
    return torch.optim.SGD([dict(params=ts, lr=lr, momentum=m, weight_decay=wd)
                            for ts, (lr, m, wd) in zip(group_lists(tensors, len(groups)), groups)], lr=0.1, **kw)


def set_lr(opt, groups, step):
    for grp, (lr, _, _) in zip(opt.param_groups, groups):           # a schedule: the learning rate changes every step
        grp['lr'] = lr * (step + 1)


@functools.lru_cache(maxsize=2)
def draw(shapes, seed, steps=STEPS):
    """-> (parameters, [gradients of step 0, 1, ...]) as fp32 CPU tensors; the gradients of step 2 (mod 4) are 100 x larger"""
    gen = torch.Generator().manual_seed(seed)
    sizes = [numel(s) for s in shapes]

    def one(scale):
        flat = torch.randn(sum(sizes), generator=gen) * scale
        return [t.reshape(s) for t, s in zip(flat.split(sizes), shapes)]
    return one(1.0), [one(10.0 if step % 4 == 2 else 0.1) for step in range(steps)]


def _strides(shape):
    mf = torch.channels_last if len(shape) == 4 else torch.contiguous_format
    return torch.empty(shape, device='meta', memory_format=mf).stride()


class Layout:
    def __init__(self, shapes, device, bucket_mb=0.05):
        slot = BucketedGradReducer._slot
        self.shapes = [tuple(s) for s in shapes]
        total = sum(slot(numel(s)) for s in self.shapes) + 2 * GUARD
        self.flat_p = torch.full((total,), SENTINEL, dtype=torch.float32, device=device)
        self.flat_b = torch.full((total,), SENTINEL, dtype=torch.float32, device=device)
        self.params, self.bufs, o = [], [], GUARD
        for s in self.shapes:
            n = numel(s)
            self.params.append(torch.nn.Parameter(self.flat_p[o:o + n].as_strided(s, _strides(s))))
            self.bufs.append(self.flat_b[o:o + n].as_strided(s, _strides(s)))
            o += slot(n)
        self.reducer = BucketedGradReducer(self.params, bucket_mb)
        self.reducer.zero_grad()            # p.grad becomes the bucket view, as at the start of a training step ...
        self.reducer.finish()               # ... and the step's bookkeeping is closed again; zero_grad() is not called any more
        self.grads = [p.grad for p in self.params]
        if self.reducer.arena is not None:
            self.flat_g = [self.reducer.arena]
        else:
            self.flat_g = [b['flat'] for b in self.reducer.buckets]
        self._flats = [('param', self.flat_p, self.params), ('momentum', self.flat_b, self.bufs)] + \
                      [('grad', f, self.grads) for f in self.flat_g]
        self._free = []
        for name, flat, views in self._flats:
            owned = torch.zeros(flat.numel(), dtype=torch.bool, device=device)
            lo, hi = flat.data_ptr(), flat.data_ptr() + 4 * flat.numel()
            for v in views:
                if lo <= v.data_ptr() < hi:
                    assert v.data_ptr() % 16 == 0
                    o = (v.data_ptr() - lo) // 4
                    assert o + v.numel() <= flat.numel() and not bool(owned[o:o + v.numel()].any())
                    owned[o:o + v.numel()] = True
            free = ~owned
            flat[free] = SENTINEL
            self._free.append(free)
        self._bits = int(torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32))

    @property
    def n_buckets(self):
        return len(self.reducer.buckets)

    def pad_floats(self):
        return sum(int(f.sum()) for f in self._free)

    def load(self, values):
        for p, v in zip(self.params, values):
            p.data.copy_(v)

    def adopt_buffers(self, opt):
        """zero-filled momentum buffers inside flat_b as the optimizer's state: what ClipSGD would create, placed by the test"""
        for p, b in zip(self.params, self.bufs):
            b.zero_()
            opt.state[p]['momentum_buffer'] = b

    def damaged(self):
        """names of the flat tensors in which a float that no view owns no longer carries SENTINEL's bits"""
        return [name for (name, flat, _), free in zip(self._flats, self._free)
                if not bool((flat.view(torch.int32)[free] == self._bits).all())]


def finite_max(t):
    return float(torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0).abs().max())


def worst_ratio(got, ref, scales):
    """max over tensors of (max |got - ref| / scale); inf where a non-finite entry of one side is not the other side's"""
    inf = float('inf')
    out = []
    for a, b in zip(got, ref):
        a, b = a.detach().double(), b.detach().double()
        same = (a == b) | (a.isnan() & b.isnan())
        d = torch.where(same, torch.zeros_like(a), (a - b).abs())
        out.append(torch.nan_to_num(d, nan=inf, posinf=inf).max())
    return float((torch.stack(out) / scales.clamp_min(1e-300)).max())


def same_values(xs, ys):
    return bool(torch.stack([((a == b) | (a.isnan() & b.isnan())).all() for a, b in zip(xs, ys)]).all())


def same_bits(xs, ys):
    return bool(torch.stack([(a.view(torch.int32) == b.view(torch.int32)).all() for a, b in zip(xs, ys)]).all())


def scalar_close(got, ref):
    if ref != ref:
        return got != got
    if ref in (float('inf'), float('-inf')):
        return got == ref
    return abs(got - ref) <= BOUND * abs(ref)


def _to_device(tensors, shapes, device):
    flat = torch.cat([t.reshape(-1) for t in tensors]).to(device)
    return [t.reshape(s) for t, s in zip(flat.split([numel(s) for s in shapes]), shapes)]


def run_case(make_plan, device, shapes, max_norm, groups=BASE, seed=11, bucket_mb=0.05, steps=STEPS, edit=None, clip_at=None,
             torch_first=0, reload_before=None, kinds=('foreach', 'fused'), bound=BOUND, log=print):
    """Runs `steps` steps of the subject in the packed layout beside the float64 reference and torch's device optimizers and
    asserts everything every case asserts; -> one record per step for what a single case asserts on top.
      edit(step, grads) -> the step's gradients (fp32 CPU tensors; must not write into its argument)
      clip_at(step, norm64) -> the step's max_norm instead of `max_norm`; the plan is rebuilt when the value changes
      torch_first: that many steps are taken by clip_grad_norm_ + optimizer.step() on the subject's own tensors first
      reload_before: the optimizer's state is reloaded from a deep copy of its state_dict before this step
    While no step has had a coefficient other than 1, parameters and buffers carry the bits of one of `kinds` (after a
    clipped step the two sides have rounded the norm differently and go on from different bits).  Seen on the MI355X: the
    foreach optimizer's bits at every such step of every case, all four steps (six when resuming) and not only the first
    two; the fused optimizer's at none (it is up to 1.7e-7 of the operands away from foreach)."""
    shapes = tuple(tuple(s) for s in shapes)
    n, G = len(shapes), len(groups)
    group_of = [i % G for i in range(n)]
    p0, grads = draw(shapes, seed, steps)
    lay = Layout(shapes, device, bucket_mb)
    lay.load(p0)
    assert not lay.damaged()
    opt = make_sgd(lay.params, groups)
    if not torch_first:
        lay.adopt_buffers(opt)
    refs = {k: [torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format)) for p in lay.params] for k in kinds}
    ropt = {k: make_sgd(refs[k], groups, **{k: True}) for k in kinds}
    P, B = [t.double() for t in p0], [None] * n
    plan, plan_norm, records, unclipped = None, None, [], True

    def state_bufs():
        return [opt.state[p]['momentum_buffer'] for p in lay.params]

    for step in range(steps):
        gs = grads[step] if edit is None else edit(step, grads[step])
        g64 = [g.double() for g in gs]
        mn = max_norm
        if clip_at is not None:
            mn = clip_at(step, float(torch.sqrt(sum((g * g).sum() for g in g64))))
        clip = None if mn is None else dict(max_norm=mn, norm_type=2)
        scales = torch.tensor([max(finite_max(p), 0.0 if b is None else finite_max(b), finite_max(g)) for p, b, g in zip(P, B, g64)],
                              dtype=torch.float64, device=device)
        gscales = torch.tensor([finite_max(g) for g in g64], dtype=torch.float64, device=device)
        gdev = _to_device(gs, shapes, device)
        for p, g in zip(lay.params, gdev):
            p.grad.copy_(g)
        for k in kinds:
            for p, g in zip(refs[k], gdev):
                p.grad = torch.empty_like(p).copy_(g)
            set_lr(ropt[k], groups, step)
        set_lr(opt, groups, step)

        if reload_before == step:
            opt.load_state_dict(copy.deepcopy(opt.state_dict()))
            assert not plan.still_valid()               # the momentum buffers are other tensors now
            plan = None
        got_norm = got_coef = None
        if step < torch_first:
            if clip is not None:
                got_norm = float(torch.nn.utils.clip_grad_norm_(lay.params, **clip))
            opt.step()
        else:
            if plan is None or mn != plan_norm:
                before = state_bufs() if step > 0 else None
                kept = None if before is None else [b.clone() for b in before]
                plan, plan_norm = make_plan(opt, clip), mn
                assert plan.ok
                if before is not None:                  # existing buffers are adopted: the same tensor objects, not zeroed
                    assert all(a is b for a, b in zip(state_bufs(), before)) and same_values(before, kept)
                    adopted = {id(e[0]): e[2] for e in plan.entries}
                    assert all(adopted[id(p)] is b for p, b in zip(lay.params, before))
            assert plan.still_valid()
            ret = plan.step()
            if clip is None:
                assert ret is None and not bool(plan.stats.any())      # no clipping: stats stay as the plan made them
            else:
                got_norm, got_coef = float(plan.stats[0]), float(plan.stats[1])
                assert float(ret) == got_norm or got_norm != got_norm
        for k in kinds:
            if clip is not None:
                torch.nn.utils.clip_grad_norm_(refs[k], **clip)
            ropt[k].step()

        P, B, Gs, norm, coef = reference_step(P, g64, B, [(lr * (step + 1), m, wd) for lr, m, wd in groups], group_of, mn)
        norm, coef = float(norm), float(coef)
        Pd, Bd, Gd = (_to_device(x, shapes, device) for x in (P, B, Gs))
        mine_p, mine_b, mine_g = [p.detach() for p in lay.params], state_bufs(), [p.grad for p in lay.params]
        rec = dict(step=step, max_norm=mn, norm=norm, coef=coef, got_norm=got_norm, got_coef=got_coef,
                   nonfinite_p=sum(int((~t.isfinite()).sum()) for t in P), nonfinite_g=sum(int((~t.isfinite()).sum()) for t in Gs),
                   err_p=worst_ratio(mine_p, Pd, scales), err_b=worst_ratio(mine_b, Bd, scales),
                   err_g=worst_ratio(mine_g, Gd, gscales), damaged=lay.damaged(), torch_err={}, versus={}, exact={})
        for k in kinds:
            tp, tb = [p.detach() for p in refs[k]], [ropt[k].state[p]['momentum_buffer'] for p in refs[k]]
            tg = [p.grad for p in refs[k]]
            rec['torch_err'][k] = max(worst_ratio(tp, Pd, scales), worst_ratio(tb, Bd, scales), worst_ratio(tg, Gd, gscales))
            rec['versus'][k] = max(worst_ratio(mine_p, tp, scales), worst_ratio(mine_b, tb, scales), worst_ratio(mine_g, tg, gscales))
            rec['exact'][k] = same_values(mine_p, tp) and same_values(mine_b, tb)
        rec['grads_untouched'] = same_bits(mine_g, gdev)
        records.append(rec)
        log('sgd case: n=%d groups=%d step=%d max_norm=%s norm=%.9g/%s coef=%.9g/%s err p=%.2e buf=%.2e g=%.2e torch=%s versus=%s exact=%s '
            'untouched=%s' % (n, G, step, mn, norm, got_norm, coef, got_coef, rec['err_p'], rec['err_b'], rec['err_g'],
                              {k: '%.2e' % v for k, v in rec['torch_err'].items()}, {k: '%.2e' % v for k, v in rec['versus'].items()},
                              rec['exact'], rec['grads_untouched']))

        assert not rec['damaged'], (step, rec['damaged'])                  # pads, gaps and guard bands: bit for bit
        assert rec['err_p'] <= bound and rec['err_b'] <= bound and rec['err_g'] <= bound, (step, rec['err_p'], rec['err_b'], rec['err_g'])
        if clip is not None:
            assert scalar_close(got_norm, norm), (step, got_norm, norm)    # (also: no SENTINEL was read)
            if got_coef is not None:
                assert scalar_close(got_coef, coef), (step, got_coef, coef)
                assert (got_coef == 1.0) == (coef == 1.0), (step, got_coef, coef)
        if coef == 1.0:
            assert rec['grads_untouched'], step
        unclipped = unclipped and coef == 1.0
        if unclipped:
            assert any(rec['exact'].values()), (step, rec['exact'])
        for k in kinds:
            assert rec['versus'][k] <= bound, (step, k, rec['versus'][k])
    return records
