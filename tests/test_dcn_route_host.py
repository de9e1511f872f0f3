"""The route of a deformable-convolution call and the workspace plan of its gather pass on the CPU, without a GPU:
tools/dcn_route_cases.cpp includes lsnet_amd/csrc/dcn_route.h -- the functions dcn.hip decides every pass's kernel with, and the
three queries of the C ABI answer from -- and checks a table of shapes around every threshold of the rule against the whole route
and plan.  A stand-alone program, built here with g++ under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FWD = ('FWD_MM', 'FWD_GROUPED', 'FWD_XN_PLANES', 'FWD_XN', 'FWD_FP32')
DATA = ('DATA_NONE', 'GATHER_GROUPED', 'GATHER_MM', 'GATHER_XN', 'SCATTER_XN', 'SCATTER_FP32')
WGRAD = ('WG_NONE', 'WG_GROUPED', 'WG_MM', 'WG_XN_ORDERED', 'WG_XN_ATOMIC', 'WG_FP32_ORDERED', 'WG_FP32_ATOMIC')
IMAGE = ('IMG_NONE', 'IMG_FRAGMENT', 'IMG_PLANES', 'IMG_PLANES_T')


def test_route_table_under_sanitizers(tmp_path):
    exe = tmp_path / 'dcn_route_cases'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           f'-I{os.path.join(ROOT, "lsnet_amd", "csrc")}', os.path.join(ROOT, 'tools', 'dcn_route_cases.cpp'),
                           '-o', str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    lines = [ln for ln in run.stdout.splitlines() if ln.strip()]
    assert len(lines) == 86 and all(ln.endswith(' ok') for ln in lines), run.stdout
    # every value of the four enums is reached: "<name>: <fwd>/<image> <data>/<image> <wgrad> ok"
    routes = [ln.rsplit(': ', 1)[1].split() for ln in lines[:-1]]
    assert {r[0].split('/')[0] for r in routes} == set(FWD)
    assert {r[1].split('/')[0] for r in routes} == set(DATA)
    assert {r[2] for r in routes} == set(WGRAD)
    assert {r[i].split('/')[1] for r in routes for i in (0, 1)} == set(IMAGE)
    # the plan's two thresholds and the gather workspace's size are cut on both sides
    for row in ('plan xn 12x12 <- 20x20 (3600 = 400 x 9 blocks): FWD_XN_PLANES/IMG_PLANES GATHER_XN/IMG_PLANES_T WG_NONE ok',
                'plan xn 12x12 <- 20x21 (3780): FWD_XN_PLANES/IMG_PLANES GATHER_XN/IMG_PLANES_T WG_NONE ok',
                'plan mm 8x8 <- 18x20 (3240 = 40 x 81 anchors): FWD_MM/IMG_FRAGMENT GATHER_MM/IMG_FRAGMENT WG_NONE ok',
                'plan mm 8x8 <- 19x20 (3420): FWD_MM/IMG_FRAGMENT GATHER_MM/IMG_FRAGMENT WG_NONE ok',
                'bwd 3x3 64->128 gather workspace of plan.bytes: FWD_MM/IMG_FRAGMENT GATHER_MM/IMG_FRAGMENT WG_NONE ok',
                'bwd 3x3 64->128 gather workspace one byte short: FWD_MM/IMG_FRAGMENT SCATTER_XN/IMG_PLANES_T WG_NONE ok',
                'wgrad 3x3 64->256: FWD_MM/IMG_FRAGMENT GATHER_MM/IMG_FRAGMENT WG_MM ok',
                'wgrad 3x3 64->256 gather workspace at offset 4: FWD_MM/IMG_FRAGMENT GATHER_MM/IMG_FRAGMENT WG_XN_ORDERED ok',
                'plan direct 8x8 <- 8192x16384 (9 x 2^27 samples): refused ok'):
        assert row in lines, row
    # every LDS threshold is cut in kh kw dg on both sides, and the grouped weight gradient at nine and ten taps
    for row in ('kd 28 = 2x7 dg 2, 64->128 (fwd_mm_lds 81920 = the cap): FWD_MM/IMG_FRAGMENT GATHER_MM/IMG_FRAGMENT WG_NONE ok',
                'kd 29 = 1x29, 64->128 (fwd_mm_lds 83968): FWD_FP32/IMG_NONE GATHER_MM/IMG_FRAGMENT WG_NONE ok',
                'kd 20 = 2x5 dg 2, 64->192 (xn_lds 163840 = the cap): FWD_XN_PLANES/IMG_PLANES GATHER_MM/IMG_FRAGMENT WG_NONE ok',
                'kd 21 = 1x21, 64->192 (xn_lds 165888): FWD_FP32/IMG_NONE GATHER_MM/IMG_FRAGMENT WG_NONE ok',
                'kd 11 = 1x11, 64->128 no gather workspace (bwd_xn_lds 80128): FWD_MM/IMG_FRAGMENT SCATTER_XN/IMG_PLANES_T WG_NONE ok',
                'kd 12 = 2x3 dg 2, 64->128 no gather workspace (bwd_xn_lds 82944): FWD_MM/IMG_FRAGMENT SCATTER_FP32/IMG_PLANES_T WG_NONE ok',
                'wgrad 1x9 512->512 64 groups (9 taps): FWD_GROUPED/IMG_NONE GATHER_GROUPED/IMG_NONE WG_GROUPED ok',
                'wgrad 2x5 512->512 64 groups (10 taps): FWD_GROUPED/IMG_NONE GATHER_GROUPED/IMG_NONE WG_XN_ORDERED ok'):
        assert row in lines, row
    # the refusal of the fp32 scatter is part of the route: the last count every route serves, and the first one it refuses
    assert sum('(bwd_fp32_lds 64-wide 163072: the last count every route serves)' in ln for ln in lines) == 1
    assert sum('(bwd_fp32_lds 64-wide 165888: refused)' in ln for ln in lines) == 1
