"""The route of a dense convolution launch on the CPU, without a GPU: tools/conv_route_cases.cpp includes
lsnet_amd/csrc/conv_route.h -- the one function conv.hip decides tile, splits and stream-K pieces with, and the piece planner it
shares with the deformable forward -- and checks a table of shapes around every threshold of the rule, plus every shape whose route
a GPU test's name or comment states.  A stand-alone program, built here with g++ under the address and undefined-behaviour
sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_route_table_under_sanitizers(tmp_path):
    exe = tmp_path / 'conv_route_cases'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           f'-I{os.path.join(ROOT, "lsnet_amd", "csrc")}', os.path.join(ROOT, 'tools', 'conv_route_cases.cpp'),
                           '-o', str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    lines = [ln for ln in run.stdout.splitlines() if ln.strip()]
    assert len(lines) == 103 and all(ln.endswith(' ok') for ln in lines), run.stdout
    # every tile and both refusals are reached
    for tile in ('128x32', '128x64', '64x128', '64x128_UNAL', '64x256', '64x256_ROWS'):
        assert any(f': {tile} ' in ln for ln in lines), tile
    assert any('refused (conv2d: C % 4 != 0 needs more than 64 output channels) ok' in ln for ln in lines)
    assert any('refused (conv2d backward-data: Co % 4 != 0 needs C > 64) ok' in ln for ln in lines)
    # what the GPU tests say they run (tests/test_stream_state_gpu.py, tests/test_ops_gpu.py)
    for ln in ('Z_SPLIT forward: 3x3 256->64 1x8x8: 128x64 1x1 ks=9 dp=1 sk=0/0 ok',
               'Z_SPLIT data gradient: 64x256 1x1 ks=2 dp=1 sk=0/0 ok',
               'STREAM_K forward: 3x3 64->128 2x65x64: 64x128 130x1 ks=1 dp=0 sk=512/130 ok',
               'STREAM_K data gradient: 128x64 65x1 ks=4 dp=65 sk=0/0 ok',
               '3x3 192->512 2x92x92 forward: 64x256 265x2 ks=1 dp=512 sk=234/18 ok',
               '3x3 192->512 2x92x92 data gradient: 64x128 265x2 ks=1 dp=512 sk=288/18 ok'):
        assert ln in lines, ln
