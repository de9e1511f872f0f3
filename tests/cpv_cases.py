"""Inputs of the corner-verification target / loss tests (tests/test_cpv_host.py, tests/test_cpv_native_gpu.py): small point
grids whose level sizes are odd or not divisible, seeded gts, one hand-made image of large boxes (so that the Gaussian bump
covers many points), and the condition the random inputs have to meet.

The positives and offsets are compared exactly.  `margins_ok` therefore states, ON THE REFERENCE SIDE (the torch statement of
core/assigners.py on the CPU), that no hard selection of a case is within reach of a rounding order:
  (a) on every level with two or more points the nearest and the second-nearest distance of every corner differ by more
      than 1e-3 px;
  (b) no |d - radius| is below 1e-3 px.
Coordinates are below 400, where a few fp32 roundings of sqrt(dx^2 + dy^2) come to ~1e-4 px.  A case that violates the
condition is replaced in the lists below, not skipped at run time (seed 2 on 100 x 120 has a tie gap of 4e-4: not listed)."""
import torch

from lsnet_amd.core import PointGenerator, PointHMAssigner
from lsnet_amd.core.assigners import gaussian_radius
from tests import golden_util as gu

STRIDES = [8, 16, 32, 64, 128]
GRID_A = (264, 376)      # levels 33x47, 17x24, 9x12, 5x6, 3x3
GRID_B = (100, 120)      # levels 13x15, 7x8, 4x4, 2x2, 1x1: a one-point level
# (image size, gt seed, number of gts)
CASES = [(GRID_A, 1, 1), (GRID_A, 2, 7), (GRID_A, 3, 40), (GRID_A, 4, 3), (GRID_A, 5, 12), (GRID_A, 6, 25),
         (GRID_B, 1, 1), (GRID_B, 7, 5)]
# large boxes: 46 / 30 bump points, 15 / 17 positives of 20 (shared cells)
LARGE_BOXES = [[13.3, 21.7, 241.9, 203.2], [15.1, 23.9, 150.6, 120.4], [190.2, 9.4, 371.3, 255.8], [60.7, 70.2, 330.1, 260.6]]
MARGIN = 1e-3


def level_sizes(hw):
    return [(-(-hw[0] // s), -(-hw[1] // s)) for s in STRIDES]


def grid(hw, device='cpu'):
    """-> points (P, 3) of an image of size hw, levels back to back"""
    pg = PointGenerator()
    return torch.cat([pg.grid_points(sz, s, device) for sz, s in zip(level_sizes(hw), STRIDES)])


def boxes_of(case):
    hw, seed, n = case
    return gu.make_gt(seed, n, hw[0], hw[1])[0]


def all_cases():
    """-> list of (name, image size, gt boxes)"""
    out = [(f'{hw[0]}x{hw[1]}_s{seed}_n{n}', hw, boxes_of((hw, seed, n))) for hw, seed, n in CASES]
    return out + [('large_boxes', GRID_A, torch.tensor(LARGE_BOXES))]


def valid_mask(P, seed=0, frac=0.7):
    return torch.rand(P, generator=gu.gen(seed)) < frac


def margins(points, boxes, gaussian_iou=0.7):
    """-> (smallest gap between the nearest and the second-nearest distance of a corner on a level with >= 2 points,
    smallest |d - radius|), torch on the CPU"""
    lvl = torch.log2(points[:, 2]).int()
    radius = gaussian_radius((boxes[:, 3] - boxes[:, 1], boxes[:, 2] - boxes[:, 0]), gaussian_iou)
    tie = rad = float('inf')
    for corner in (boxes[:, :2], boxes[:, 2:]):
        dist = (points[:, None, :2] - corner[None]).norm(dim=2)
        rad = min(rad, float((dist - radius[None]).abs().min()))
        for l in lvl.unique().tolist():
            d = dist[lvl == l]
            if d.shape[0] < 2:
                continue
            v = d.topk(2, dim=0, largest=False)[0]
            tie = min(tie, float((v[1] - v[0]).min()))
    return tie, rad


def margins_ok(points, boxes, gaussian_iou=0.7):
    tie, rad = margins(points, boxes, gaussian_iou)
    return tie > MARGIN and rad > MARGIN


def statement(pts, valid, boxes, bump):
    """PointHMAssigner.assign_dense on the valid points, scattered back over all points as LSCPVHead.get_hm_targets does
    -> hm (2, P) float, off (2, P, 2)"""
    sub = pts if valid is None else pts[valid]
    hm_tl, off_tl, hm_br, off_br = PointHMAssigner(bump, 0.7).assign_dense(sub, boxes, strides=STRIDES)
    hm, off = torch.stack([hm_tl, hm_br]).float(), torch.stack([off_tl, off_br])
    if valid is None:
        return hm, off
    full_hm, full_off = pts.new_zeros(2, len(pts)), pts.new_zeros(2, len(pts), 2)
    full_hm[:, valid], full_off[:, valid] = hm, off
    return full_hm, full_off


def same_targets(got, want, what):
    """positives, their count and offsets exact; the heat-map within 5e-6 relative: its exponent is below 4.5 in magnitude
    (d < r and sigma = (2 r + 1) / 6), carries <= 6 roundings, and exp is a few ulp on each side"""
    hm, off, npos = got
    assert torch.equal(hm == 1, want[0] == 1), what
    assert torch.equal(npos.long(), (want[0] == 1).sum(1)), what
    assert torch.equal(off, want[1]), what
    assert torch.equal(hm == 0, want[0] == 0), what
    assert ((hm - want[0]).abs() <= 5e-6 * want[0].abs()).all(), what


def judge(native, torch32, ref64, what):
    """The rule of the loss comparisons: both fp32 arms against a float64 evaluation of the same formulas on the same inputs.
    The error is the largest element-wise deviation, scaled by the largest reference magnitude (for a loss value: its own);
    the native arm's may be at most twice the torch statement's, or 16 ulp (1e-6 relative) where that is larger.
    -> (native error, torch error), printed for the records."""
    ref64 = ref64.detach().double().cpu()
    scale = float(ref64.abs().max()) if ref64.numel() else 0.0
    if scale == 0.0 or ref64.numel() == 0:
        assert not native.detach().cpu().double().abs().any(), what
        return 0.0, 0.0
    e_n = float((native.detach().double().cpu() - ref64).abs().max()) / scale
    e_t = float((torch32.detach().double().cpu() - ref64).abs().max()) / scale
    print(f'{what}: native {e_n:.3e}  torch fp32 {e_t:.3e}  (scale {scale:.4g})')
    assert e_n <= max(2 * e_t, 1e-6), (what, e_n, e_t)
    return e_n, e_t
