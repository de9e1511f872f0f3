"""The corner verification of the decode kernels (decode_box_verified of lsnet_amd/csrc/decode_rows.h, shared with
csrc/decode.hip) against the torch statements of LSCPVHead.get_bboxes, without a GPU: the header is compiled here with g++ under
the loop-nest driver of tests/test_decode_host.py, whose box step verifies the corners of a level that has a source.  Inputs
and reference: tests/cpv_decode_cases.py.  Boxes, labels and order are held np.array_equal; scores within 1e-6."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import cpv_decode_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = r'''
#include <algorithm>
#include <vector>
#include "decode_rows.h"

static DecodeMap dense(const float *p, int H, int W)
{
    DecodeMap m;
    m.base = p, m.sc = (int64_t)H * W, m.sy = W, m.sx = 1;
    return m;
}

// one image; maps are dense (channels, H, W) arrays per level; source s is level s (its heat-map, offsets, stride and size)
extern "C" int decode_cpv_image(int L, const int *H, const int *W, const float *stride, const float *const *cls,
                                const float *const *box, const float *const *heat, const float *const *off, const int *verify,
                                int C, float img_h, float img_w, const float *sf, int nms_pre, float score_thr, float iou_thr,
                                int class_agnostic, int max_per_img, float *dets, long long *labels)
{
    struct Slot { int level, row; };
    std::vector<Slot> slots;
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
    std::vector<float> boxes(slots.size() * 4);
    std::vector<uint64_t> cand;
    float maxc = 0.f;
    for (size_t s = 0; s < slots.size(); ++s) {
        const int l = slots[s].level, y = slots[s].row / W[l], x = slots[s].row % W[l];
        bool any = false;
        for (int c = 0; c < C; ++c) {
            const float score = decode_sigmoid(decode_at(dense(cls[l], H[l], W[l]), c, y, x));
            if (!(score > score_thr)) continue;
            if (!any) {
                DecodeGeom g;
                g.stride = stride[l], g.img_w = img_w, g.img_h = img_h;
                for (int i = 0; i < 4; ++i) g.sf[i] = sf[i];
                DecodeCorner corner;
                const int v = verify[l];
                if (v >= 0) {
                    corner.heat = dense(heat[v], H[v], W[v]), corner.off = dense(off[v], H[v], W[v]);
                    corner.H = H[v], corner.W = W[v], corner.stride = stride[v];
                }
                decode_box_verified(dense(box[l], H[l], W[l]), y, x, g, v >= 0 ? &corner : nullptr, &boxes[s * 4]);
                for (int i = 0; i < 4; ++i) maxc = boxes[s * 4 + i] > maxc ? boxes[s * 4 + i] : maxc;
                any = true;
            }
            cand.push_back(decode_order_key(score, (uint32_t)(s * C + c)));
        }
    }
    std::sort(cand.begin(), cand.end());
    std::vector<float> kept;
    int nk = 0;
    for (size_t i = 0; i < cand.size() && nk < max_per_img; ++i) {
        const uint32_t id = decode_order_id(cand[i]), s = id / C, c = id % C;
        const float o = class_agnostic ? 0.f : decode_nms_offset((int)c, maxc);
        float b[4];
        for (int q = 0; q < 4; ++q) b[q] = boxes[s * 4 + q] + o;
        bool alive = true;
        for (int q = 0; q < nk && alive; ++q) alive = !decode_iou_gt(&kept[q * 4], b, iou_thr);
        if (!alive) continue;
        kept.insert(kept.end(), b, b + 4);
        for (int q = 0; q < 4; ++q) dets[nk * 5 + q] = boxes[s * 4 + q];
        dets[nk * 5 + 4] = decode_order_score(cand[i]);
        labels[nk] = c;
        ++nk;
    }
    return nk;
}

// the unverified route and decode_box give the same bits
extern "C" int same_as_decode_box(const float *box, int H, int W, int y, int x, float stride, float img_h, float img_w, const float *sf)
{
    DecodeGeom g;
    g.stride = stride, g.img_w = img_w, g.img_h = img_h;
    for (int i = 0; i < 4; ++i) g.sf[i] = sf[i];
    float a[4], b[4];
    decode_box(dense(box, H, W), 0, 4, y, x, g, a);
    decode_box_verified(dense(box, H, W), y, x, g, nullptr, b);
    union { float f; uint32_t u; } p, q;
    for (int i = 0; i < 4; ++i) {
        p.f = a[i], q.f = b[i];
        if (p.u != q.u) return 0;
    }
    return 1;
}

extern "C" int corner_cell(float v, float s, int n) { return decode_corner_cell(v, s, n); }
'''

F32 = ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp('decode_cpv')
    src = d / 'driver.cpp'
    src.write_text(DRIVER)
    so = d / 'decode_cpv.so'
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off',
                           f'-I{os.path.join(ROOT, "lsnet_amd", "csrc")}', str(src), '-o', str(so)])
    return ctypes.CDLL(str(so))


def run_driver(lib, outs, cfg, scale_factors=None, img=cc.IMG):
    h = cc.head()
    B, L = outs[0][0].shape[0], len(outs[0])
    Hs = (ctypes.c_int * L)(*[t.shape[2] for t in outs[0]])
    Ws = (ctypes.c_int * L)(*[t.shape[3] for t in outs[0]])
    strides = (ctypes.c_float * L)(*[float(s) for s in h.point_strides[:L]])
    verify = (ctypes.c_int * L)(*h._verify_sources(L))
    res = []
    for b in range(B):
        keep = [[np.ascontiguousarray(t[b].numpy(), dtype=np.float32) for t in outs[k]] for k in (0, 2, 3, 4)]
        ptrs = [(F32 * L)(*[a.ctypes.data_as(F32) for a in lst]) for lst in keep]
        sf = np.ones(4, np.float32) if scale_factors is None else np.asarray(scale_factors, np.float32)
        m = cfg.max_per_img
        dets, labels = np.zeros((m, 5), np.float32), np.zeros(m, np.int64)
        n = lib.decode_cpv_image(L, Hs, Ws, strides, ptrs[0], ptrs[1], ptrs[2], ptrs[3], verify, cc.CLASSES,
                                 ctypes.c_float(img[0]), ctypes.c_float(img[1]), sf.ctypes.data_as(F32), cfg.get('nms_pre', -1),
                                 ctypes.c_float(cfg.score_thr), ctypes.c_float(cfg.nms['iou_thr']),
                                 int(bool(cfg.nms.get('class_agnostic', False))), m, dets.ctypes.data_as(F32),
                                 labels.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
        res.append((dets[:n], labels[:n]))
    return res


def test_driver_matches_the_torch_statements(rows):
    outs, full, cut, tight = cc.reference()
    worst = cc.assert_same(run_driver(rows, outs, cc.config()), full, 'cpv')
    worst = max(worst, cc.assert_same(run_driver(rows, outs, cc.config(max_per_img=10)), cut, 'cpv cut'))
    worst = max(worst, cc.assert_same(run_driver(rows, outs, cc.config(nms=dict(iou_thr=0.1))), tight, 'cpv iou 0.1'))
    print(f'largest score difference {worst:.3e}')


def test_all_points_of_every_level(rows):
    """nms_pre = -1: no top-k, every point with a candidate is verified."""
    outs = cc.reference()[0]
    cfg = cc.config(nms_pre=-1)
    cc.assert_same(run_driver(rows, outs, cfg), cc.torch_path(outs, cfg), 'cpv all points')


def test_rescale_and_class_agnostic(rows):
    """The division by the scale factors comes after the snap, per coordinate."""
    outs, full = cc.reference()[:2]
    for sf, four in ((1.5, [1.5] * 4), (np.array([1.25, 1.5, 1.75, 2.0], np.float32), [1.25, 1.5, 1.75, 2.0])):
        want = cc.torch_path(outs, cc.config(), rescale=True, scale_factor=sf)
        assert all(len(w[0]) for w in want)
        cc.assert_same(run_driver(rows, outs, cc.config(), four), want, f'cpv scale {four}')
    cfg = cc.config(nms=dict(class_agnostic=True))
    want = cc.torch_path(outs, cfg)
    assert sum(len(w[0]) for w in want) < sum(len(w[0]) for w in full), 'class-agnostic NMS suppresses no more than per-class NMS'
    cc.assert_same(run_driver(rows, outs, cfg), want, 'cpv class-agnostic')


def test_unverified_level_keeps_the_bits_of_decode_box(rows):
    outs = cc.reference()[0]
    sf = np.array([1.25, 1.5, 1.75, 2.0], np.float32)
    for l, (H, W) in enumerate(cc.GRIDS):
        m = np.ascontiguousarray(outs[2][l][0].numpy())
        for y in range(H):
            for x in range(W):
                assert rows.same_as_decode_box(m.ctypes.data_as(F32), H, W, y, x, ctypes.c_float(8 << l), ctypes.c_float(cc.IMG[0]),
                                               ctypes.c_float(cc.IMG[1]), sf.ctypes.data_as(F32))


def test_cell_index_never_leaves_the_map(rows):
    """floor(clamp(v / s, 0, n - 2)) for ordinary values; 0 .. n - 2 for a NaN, an infinity and values beyond the int range."""
    cell = rows.corner_cell
    for v, s, n, want in ((0.0, 8.0, 9, 0), (7.99, 8.0, 9, 0), (8.0, 8.0, 9, 1), (55.9, 8.0, 9, 6), (56.0, 8.0, 9, 7),
                          (63.9, 8.0, 9, 7), (1000.0, 8.0, 9, 7), (-3.0, 8.0, 9, 0), (5.0, 16.0, 2, 0), (500.0, 16.0, 2, 0)):
        assert cell(ctypes.c_float(v), ctypes.c_float(s), n) == want, (v, s, n)
    for v in (float('nan'), float('inf'), float('-inf'), 3e38, -3e38):
        for n in (2, 3, 9):
            assert 0 <= cell(ctypes.c_float(v), ctypes.c_float(8.0), n) <= n - 2, (v, n)


def test_library_argument_checks_need_no_gpu():
    from lsnet_amd import _lib
    lib = _lib.load()
    lv = (_lib.DecodeLevel * 2)()
    lv[0].H, lv[0].W, lv[1].H, lv[1].W = 9, 13, 6, 8
    src = (_lib.DecodeSource * 2)()
    src[0].H, src[0].W, src[1].H, src[1].W = 9, 13, 1, 8
    src[0].heat = src[0].offset = src[1].heat = src[1].offset = 16      # (never read: an argument check ends every call here)
    tail = (8, None, None, 12, 0.05, 0.6, 0, 100, 16384, None, None, None, None, None)
    assert lib.lsn_decode_cpv_batch(3, 2, lv, 2, src, (ctypes.c_int * 2)(-1, 0), *tail) == -1
    assert b'corner source 1 is 1 x 8' in lib.lsn_last_error()
    src[1].H = 6
    for bad in (2, -2):
        assert lib.lsn_decode_cpv_batch(3, 2, lv, 2, src, (ctypes.c_int * 2)(-1, bad), *tail) == -1
        assert f'source {bad} of 2'.encode() in lib.lsn_last_error()
    assert lib.lsn_decode_cpv_batch(3, 2, lv, 9, src, (ctypes.c_int * 2)(-1, 0), *tail) == -1
    assert b'9 corner sources' in lib.lsn_last_error()
