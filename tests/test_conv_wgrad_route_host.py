"""The route of the dense convolution's weight gradient on the CPU, without a GPU: tools/conv_wgrad_route_cases.cpp includes
lsnet_amd/csrc/conv_wgrad_route.h -- the one function the library decides with -- and checks a table of shapes around every
threshold of the rule.  A stand-alone program, built here with g++ under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_route_table_under_sanitizers(tmp_path):
    exe = tmp_path / 'conv_wgrad_route_cases'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           f'-I{os.path.join(ROOT, "lsnet_amd", "csrc")}', os.path.join(ROOT, 'tools', 'conv_wgrad_route_cases.cpp'),
                           '-o', str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    lines = [ln for ln in run.stdout.splitlines() if ln.strip()]
    assert len(lines) == 25 and all(ln.endswith(' ok') for ln in lines), run.stdout
    # every route is reached, and the two pixel thresholds are cut on both sides
    for route in ('DENSE_MM', 'PATCH', 'PATCH_JOBS', 'GENERAL'):
        assert any(ln.endswith(f': {route} ok') for ln in lines), route
    assert any(ln == '3x3 s1 64->256 1x64x64 (4096 px): DENSE_MM ok' for ln in lines)
    assert any(ln == '3x3 s1 64->256 1x63x65 (4095 px): PATCH ok' for ln in lines)
    assert any(ln == '1x1 s1 1024->512 1x23x89 (2047 px): PATCH ok' for ln in lines)
