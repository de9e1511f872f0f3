"""The anchor-list sort of the deformable backward on the CPU, without a GPU: tools/dcn_sort_emul.cpp walks the blocks, waves,
rows and lanes of the device kernels one after the other on the arithmetic they share with it (lsnet_amd/csrc/dcn_sort_plan.h:
digit widths, pass count, sentinel, histogram layout, position formula), with every array sized as the library sizes it, and
compares each case with std::stable_sort.  It is a stand-alone program, built here with g++ under the address and
undefined-behaviour sanitizers: a scatter position outside the output is a heap overflow in this run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sort_emulation_under_sanitizers(tmp_path):
    exe = tmp_path / 'dcn_sort_emul'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           f'-I{os.path.join(ROOT, "lsnet_amd", "csrc")}', os.path.join(ROOT, 'tools', 'dcn_sort_emul.cpp'),
                           '-o', str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    lines = [ln for ln in run.stdout.splitlines() if ln.strip()]
    assert len(lines) >= 17 and all(' ok: ' in ln for ln in lines), run.stdout
    # the cases the digit plan has to get right: 16 + 1 bits, the widest two-pass digits, three passes
    assert any('65536 anchors, 2 passes x  9 bits' in ln for ln in lines)
    assert any('4194303 anchors, 2 passes x 11 bits' in ln for ln in lines)
    assert any('4194304 anchors, 3 passes x  8 bits' in ln for ln in lines)
    assert any('1073741823 anchors, 3 passes x 10 bits' in ln for ln in lines)
