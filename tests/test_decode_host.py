"""The row arithmetic of the decode kernels (lsnet_amd/csrc/decode_rows.h, shared with csrc/decode.hip) against the torch
statements of LSHead.get_bboxes, without a GPU: the header is compiled here with g++ under a loop-nest driver that states the
six steps the way the kernels do -- select per level (largest keys, equal keys to the lower row), decode of the selected
points only, candidates above score_thr, the total order (score descending, then level, row, class), greedy NMS against a kept
list that stops at max_per_img, emit.  Inputs: tests/decode_cases.py.

Labels, order and coordinates are held np.array_equal; scores within 1e-6.  Largest score difference seen between glibc's expf
form and torch's CPU sigmoid over all cases here: 1.2e-7 (5.96e-8 = one ulp below 1 is the typical difference)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import decode_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = r'''
#include <algorithm>
#include <vector>
#include "decode_rows.h"

// one image; maps are dense (channels, H, W) arrays per level
extern "C" int decode_image(int L, const int *H, const int *W, const float *stride, const float *const *cls,
                            const float *const *box, const float *const *vec, int C, int nv, int kind, float img_h, float img_w,
                            const float *sf, int nms_pre, float score_thr, float iou_thr, int class_agnostic, int max_per_img,
                            float *dets, float *vecs, long long *labels)
{
    struct Slot { int level, row; };
    std::vector<Slot> slots;
    // 1. select
    for (int l = 0; l < L; ++l) {
        const int P = H[l] * W[l];
        std::vector<int> rows(P);
        for (int i = 0; i < P; ++i) rows[i] = i;
        if (nms_pre > 0 && nms_pre < P) {
            std::vector<uint32_t> key(P);
            for (int i = 0; i < P; ++i) {
                float best = decode_sigmoid(cls[l][i]);
                for (int c = 1; c < C; ++c) best = decode_max(best, decode_sigmoid(cls[l][(size_t)c * P + i]));
                key[i] = decode_key(best);
            }
            std::sort(rows.begin(), rows.end(), [&](int a, int b) { return key[a] != key[b] ? key[a] > key[b] : a < b; });
            rows.resize(nms_pre);
            std::sort(rows.begin(), rows.end());
        }
        for (int r : rows) slots.push_back({l, r});
    }
    // 2. decode the selected points, 3. candidates
    auto geom = [&](int l) {
        DecodeGeom g;
        g.stride = stride[l], g.img_w = img_w, g.img_h = img_h;
        for (int i = 0; i < 4; ++i) g.sf[i] = sf[i];
        return g;
    };
    auto map = [&](const float *p, int l) {
        DecodeMap m;
        m.base = p, m.sc = (int64_t)H[l] * W[l], m.sy = W[l], m.sx = 1;
        return m;
    };
    std::vector<float> boxes(slots.size() * 4);
    std::vector<uint64_t> cand;
    float maxc = 0.f;
    for (size_t s = 0; s < slots.size(); ++s) {
        const int l = slots[s].level, y = slots[s].row / W[l], x = slots[s].row % W[l];
        bool any = false;
        for (int c = 0; c < C; ++c) {
            const float score = decode_sigmoid(decode_at(map(cls[l], l), c, y, x));
            if (!(score > score_thr)) continue;
            if (!any) {
                decode_box(map(box[l], l), kind == DECODE_VECTORS, nv, y, x, geom(l), &boxes[s * 4]);
                for (int i = 0; i < 4; ++i) maxc = boxes[s * 4 + i] > maxc ? boxes[s * 4 + i] : maxc;
                any = true;
            }
            cand.push_back(decode_order_key(score, (uint32_t)(s * C + c)));
        }
    }
    // 4. order
    std::sort(cand.begin(), cand.end());
    // 5. greedy NMS against the kept list, 6. emit
    std::vector<float> kept;
    int nk = 0;
    for (size_t i = 0; i < cand.size() && nk < max_per_img; ++i) {
        const uint32_t id = decode_order_id(cand[i]), s = id / C, c = id % C;
        const float off = class_agnostic ? 0.f : decode_nms_offset((int)c, maxc);
        float b[4];
        for (int q = 0; q < 4; ++q) b[q] = boxes[s * 4 + q] + off;
        bool alive = true;
        for (int q = 0; q < nk && alive; ++q) alive = !decode_iou_gt(&kept[q * 4], b, iou_thr);
        if (!alive) continue;
        kept.insert(kept.end(), b, b + 4);
        const int l = slots[s].level, y = slots[s].row / W[l], x = slots[s].row % W[l];
        for (int q = 0; q < 4; ++q) dets[nk * 5 + q] = boxes[s * 4 + q];
        dets[nk * 5 + 4] = decode_order_score(cand[i]);
        labels[nk] = c;
        for (int q = 0; q < 2 * nv; ++q)
            vecs[nk * 2 * nv + q] = decode_vec(map(vec[l], l), kind, q, y, x, geom(l), &boxes[s * 4]);
        ++nk;
    }
    return nk;
}

extern "C" float key_roundtrip(float v) { return decode_key_value(decode_key(v)); }
extern "C" unsigned long long order_key(float score, unsigned id) { return decode_order_key(score, id); }
'''

F32 = ctypes.POINTER(ctypes.c_float)
KINDS = {'bbox': 0, 'segm': 1, 'pose_kbox': 1, 'pose_bbox': 2}


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp('decode')
    src = d / 'driver.cpp'
    src.write_text(DRIVER)
    so = d / 'decode.so'
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off',
                           f'-I{os.path.join(ROOT, "lsnet_amd", "csrc")}', str(src), '-o', str(so)])
    lib = ctypes.CDLL(str(so))
    lib.key_roundtrip.restype = ctypes.c_float
    lib.order_key.restype = ctypes.c_ulonglong
    return lib


def run_driver(lib, task, outs, cfg, scale_factors=None, num_classes=dc.CLASSES, img=dc.IMG):
    h = dc.head(task, num_classes)
    nv = h.num_vectors
    box_src, vec_src = h._decode_sources(outs[2], outs[4], outs[6])
    B, L = outs[0][0].shape[0], len(outs[0])
    Hs = (ctypes.c_int * L)(*[t.shape[2] for t in outs[0]])
    Ws = (ctypes.c_int * L)(*[t.shape[3] for t in outs[0]])
    strides = (ctypes.c_float * L)(*[float(s) for s in h.point_strides[:L]])
    res = []
    for b in range(B):
        keep = [[np.ascontiguousarray(t[b].numpy(), dtype=np.float32) for t in src] for src in (outs[0], box_src, vec_src)]
        ptrs = [(F32 * L)(*[a.ctypes.data_as(F32) for a in lst]) for lst in keep]
        sf = np.ones(4, np.float32) if scale_factors is None else np.asarray(scale_factors, np.float32)
        m = cfg.max_per_img
        dets, vecs, labels = np.zeros((m, 5), np.float32), np.zeros((m, 2 * nv), np.float32), np.zeros(m, np.int64)
        n = lib.decode_image(L, Hs, Ws, strides, ptrs[0], ptrs[1], ptrs[2], num_classes, nv, KINDS[task],
                             ctypes.c_float(img[0]), ctypes.c_float(img[1]), sf.ctypes.data_as(F32), cfg.get('nms_pre', -1),
                             ctypes.c_float(cfg.score_thr), ctypes.c_float(cfg.nms['iou_thr']),
                             int(bool(cfg.nms.get('class_agnostic', False))), m, dets.ctypes.data_as(F32), vecs.ctypes.data_as(F32),
                             labels.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
        res.append((dets[:n], vecs[:n], labels[:n]))
    return res


@pytest.mark.parametrize('task', dc.TASKS)
def test_driver_matches_the_torch_statements(rows, task):
    outs, full, cut, tight = dc.reference(task)
    worst = dc.assert_same(run_driver(rows, task, outs, dc.config()), full, task)
    worst = max(worst, dc.assert_same(run_driver(rows, task, outs, dc.config(max_per_img=10)), cut, task + ' cut'))
    worst = max(worst, dc.assert_same(run_driver(rows, task, outs, dc.config(nms=dict(iou_thr=0.1))), tight, task + ' iou 0.1'))
    print(f'{task}: largest score difference {worst:.3e}')


@pytest.mark.parametrize('task', dc.TASKS)
def test_rescale_and_class_agnostic(rows, task):
    outs, full = dc.reference(task)[:2]
    for sf, four in ((1.5, [1.5] * 4), (np.array([1.25, 1.5, 1.75, 2.0], np.float32), [1.25, 1.5, 1.75, 2.0])):
        want = dc.torch_path(task, outs, dc.config(), rescale=True, scale_factor=sf)
        assert all(len(w[0]) for w in want)
        dc.assert_same(run_driver(rows, task, outs, dc.config(), four), want, f'{task} scale {four}')
    cfg = dc.config(nms=dict(class_agnostic=True))
    want = dc.torch_path(task, outs, cfg)
    assert sum(len(w[0]) for w in want) < sum(len(w[0]) for w in full), 'class-agnostic NMS suppresses no more than per-class NMS'
    dc.assert_same(run_driver(rows, task, outs, cfg), want, f'{task} class-agnostic')


@pytest.mark.parametrize('classes', [1, 80])
def test_class_counts(rows, classes):
    outs, gap = dc.inputs('bbox', seed=9, num_classes=classes)
    assert gap > 1e-3
    want = dc.torch_path('bbox', outs, dc.config(), num_classes=classes)
    assert all(len(w[0]) for w in want)
    dc.assert_same(run_driver(rows, 'bbox', outs, dc.config(), num_classes=classes), want, f'C={classes}')


def test_sizes_at_which_the_kernels_change_path(rows):
    """The references of the large GPU cases (a level of 16 800 points under nms_pre = 1000 with 1048 candidates; 8520 candidates
    in an image) hold for the loop nest too."""
    outs, cfg, want = dc.big_select_case()
    dc.assert_same(run_driver(rows, 'bbox', outs, cfg, num_classes=1, img=dc.BIG_IMG), want, 'large level')
    outs, cfg, want = dc.big_sort_case()
    dc.assert_same(run_driver(rows, 'bbox', outs, cfg, num_classes=40), want, 'many candidates')


def test_order_key_states_the_tie_rule(rows):
    """Descending score, then ascending id; the score comes back from the word bit for bit."""
    k = rows.order_key
    assert k(ctypes.c_float(0.9), 7) < k(ctypes.c_float(0.5), 0)
    assert k(ctypes.c_float(0.5), 3) < k(ctypes.c_float(0.5), 4)
    for v in np.array([0.0, 1e-30, 0.05, 0.5, 1.0], np.float32):
        assert np.float32(rows.key_roundtrip(ctypes.c_float(v))) == v


def test_library_argument_checks_need_no_gpu():
    from lsnet_amd import _lib
    lib = _lib.load()
    lv = (_lib.DecodeLevel * 2)()
    lv[0].H, lv[0].W, lv[1].H, lv[1].W = 100, 168, 3, 4
    # keys of the level above the top-k, one select row and one box per slot, the candidate words
    assert lib.lsn_decode_workspace_bytes(4, 2, lv, 1000, 16384) >= 4 * (16800 * 4 + 1012 * 20 + 16384 * 8)
    assert lib.lsn_decode_workspace_bytes(65, 2, lv, 1000, 16384) == -1
    assert b'65 images' in lib.lsn_last_error()
    assert lib.lsn_decode_batch(4, 9, lv, 1, None, None, 4, 0, 1000, 0.05, 0.6, 0, 100, 16384, None, None, None, None, None,
                                None) == -1
