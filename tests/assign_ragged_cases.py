"""Inputs of the ragged-batch assignment tests (tests/test_assign_ragged_host.py, tests/test_assign_ragged_gpu.py): images of
`assign_cases.CASES` whose valid region is smaller than the 800 x 800 grid, the reference-side statement of what a masked
batched call has to give (the torch assigner on the FILTERED points / boxes with the shortened levels, scattered back into
the full grid -- the `inside_flags` path of lsnet_head.py:810-917), and the same for the per-point targets.

The comparisons are exact, so every image meets `assign_cases.margins_ok` on its filtered, reference-side inputs for
topk = 9 and the three CENTROID_MODES (asserted in the host test).  A case that fails is replaced here, not skipped."""
import torch

from lsnet_amd.core import ATSSAssigner, CentroidAssigner, PointGenerator
from tests import assign_cases as ac
from tests import golden_util as gu

TOPK = 9
# index in assign_cases.CASES -> the valid region (h, w), the valid cells per level it leaves and the gts kept (x2 < w, y2 < h)
IMAGES = {
    0: ((800, 800), [10000, 2500, 625, 169, 49], 7),
    1: ((600, 700), [6600, 1672, 418, 110, 30], 7),
    12: ((576, 736), [6624, 1656, 414, 108, 30], 15),
    3: ((480, 800), [6000, 1500, 375, 104, 28], 4),
    4: ((704, 512), [5632, 1408, 352, 88, 24], 10),
}
BATCHES = [[0, 1, 12], [3, 4, None]]        # None: an image without gts (the region of CASES[1], its proposals)


def region_flags(h, w, device='cpu'):
    """-> ((P,) bool flags of the grid cells inside an h x w image, their count per level)"""
    _, sizes = ac.grid()
    pg = PointGenerator()
    valid = [(min(sz[0], -(-h // s)), min(sz[1], -(-w // s))) for sz, s in zip(sizes, ac.STRIDES)]
    flags = torch.cat([pg.valid_flags(sz, v, device) for sz, v in zip(sizes, valid)])
    return flags, [v[0] * v[1] for v in valid]


def image(index):
    """-> dict of CPU tensors: pts (P, 3), level_len, flags (P,), counts, boxes / labels / extremes of the gts kept, props (P, 4)"""
    pts, sizes = ac.grid()
    src = 1 if index is None else index
    (h, w), _, _ = IMAGES[src]
    seed, ng, pseed, _, _ = ac.CASES[src]
    b, l, e = gu.make_gt(seed, ng, 800, 800)
    keep = (b[:, 2] < w) & (b[:, 3] < h)
    if index is None:
        keep = torch.zeros_like(keep)
    flags, counts = region_flags(h, w)
    return dict(pts=pts, level_len=[s[0] * s[1] for s in sizes], flags=flags, counts=counts, boxes=b[keep], labels=l[keep],
                extremes=e[keep], props=ac.proposals(pts, pseed))


def margins_ok(im):
    f = im['flags']
    return ac.margins_ok(im['pts'][f], [(n, 1) for n in im['counts']], im['boxes'], im['extremes'], im['props'][f], (TOPK,))


def scatter(flags, v, fill):
    out = v.new_full((flags.numel(),) + tuple(v.shape[1:]), fill)
    out[flags] = v
    return out


def centroid_statement(im, pos_num, typ, with_labels=True):
    """-> (gt_inds (P,), labels (P,) or None) over the full grid"""
    f, P = im['flags'], len(im['pts'])
    if len(im['boxes']) == 0:
        return torch.zeros(P, dtype=torch.long, device=f.device), (torch.full((P,), -1, device=f.device) if with_labels else None)
    res = CentroidAssigner(scale=4, pos_num=pos_num, iou_type=typ).assign(im['pts'][f], im['boxes'], im['extremes'], None,
                                                                          im['labels'] if with_labels else None)
    return scatter(f, res.gt_inds, 0), (scatter(f, res.labels, -1) if with_labels else None)


def atss_statement(im, props=None, with_labels=True):
    """-> (gt_inds, max_overlaps with -1e8 outside the image, labels or None) over the full grid"""
    f, P = im['flags'], len(im['pts'])
    props = im['props'] if props is None else props
    if len(im['boxes']) == 0:
        return torch.zeros(P, dtype=torch.long, device=f.device), torch.full((P,), -1e8, device=f.device), \
            (torch.full((P,), -1, device=f.device) if with_labels else None)
    res = ATSSAssigner(topk=TOPK).assign(props[f], im['counts'], im['boxes'], None, im['labels'] if with_labels else None)
    return scatter(f, res.gt_inds, 0), scatter(f, res.max_overlaps, -1e8), (scatter(f, res.labels, -1) if with_labels else None)


def targets_statement(gt_inds, flags, table, gt_labels, background):
    """One image: the statements of LSHead._dense_targets on the filtered points, then the scatter of LSHead._assign_image.
    -> rows (P, D), labels (P,), label_weights (P,), bbox_weights (P, 4), num_pos"""
    gi = gt_inds[flags]
    pos = gi > 0
    idx = (gi - 1).clamp(min=0)
    if table.shape[0] == 0:             # the "nothing to assign" branch: all background
        rows = table.new_zeros((len(gi), table.shape[1]))
        labels = torch.full_like(gi, background)
    else:
        rows = torch.where(pos[:, None], table[idx], 0.0)
        labels = torch.where(pos, gt_labels[idx] if gt_labels is not None else torch.ones_like(idx), background)
    bw = pos[:, None].to(table.dtype).expand(-1, 4)
    lw = torch.ones_like(pos, dtype=table.dtype)
    return scatter(flags, rows, 0), scatter(flags, labels, 0), scatter(flags, lw, 0), scatter(flags, bw, 0), pos.sum()


def seeded_gt_inds(seed, flags, G):
    """~5 % positives among the valid points, as tests/test_assign_gpu.py::test_dense_targets draws them; 0 outside the image"""
    g = gu.gen(seed)
    P = flags.numel()
    if G == 0:
        return torch.zeros(P, dtype=torch.long)
    draw = torch.where(torch.rand(P, generator=g) < 0.05, torch.randint(1, G + 1, (P,), generator=g), 0)
    return torch.where(flags, draw, 0)
