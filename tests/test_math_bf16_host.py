"""The single-product bf16 math mode ('bf16', LSN_MATH_BF16) on the host side: the C ABI round trip, the LSNET_MATH
switch, and the mapping of mmdet's `fp16` config key onto it (lsnet_amd/apis/train.py).  The built library, no GPU."""
import os
import subprocess
import sys

import pytest

from lsnet_amd import _lib
from lsnet_amd.apis.train import config_math_mode, math_mode_of
from lsnet_amd.utils import ConfigDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def restore_mode():
    before = _lib.get_math_mode()
    yield before
    _lib.set_math_mode(before)


def test_set_and_get_bf16(restore_mode):
    _lib.set_math_mode('bf16')
    assert _lib.get_math_mode() == 'bf16'
    assert _lib.load().lsn_get_math_mode() == _lib.MATH_BF16 == 3
    assert _lib.split_math()
    for mode in ('bf16x6', 'bf16x3', 'fp32', 'bf16'):
        _lib.set_math_mode(mode)
        assert _lib.get_math_mode() == mode


def test_unknown_mode_is_refused(restore_mode):
    _lib.set_math_mode('bf16')
    with pytest.raises(RuntimeError, match='unknown math mode'):
        _lib.set_math_mode(4)
    assert _lib.get_math_mode() == 'bf16'


def test_environment_selects_bf16():
    env = dict(os.environ, LSNET_MATH='bf16')
    out = subprocess.run([sys.executable, '-c', 'from lsnet_amd import _lib; print(_lib.get_math_mode())'], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == 'bf16'


def test_fp16_config_key_maps_to_bf16(restore_mode):
    _lib.set_math_mode('bf16x3')
    lines = []
    cfg = ConfigDict(dict(fp16=dict(loss_scale=512.), total_epochs=1))
    assert math_mode_of(cfg) == 'bf16'
    with config_math_mode(cfg, lines.append) as mode:
        assert mode == 'bf16' and _lib.get_math_mode() == 'bf16'
    assert _lib.get_math_mode() == 'bf16x3'        # the previous mode is back
    assert len(lines) == 1
    assert 'bf16 products' in lines[0] and 'fp32 accumulation' in lines[0] and 'stay fp32' in lines[0]
    assert 'loss_scale=512.0' in lines[0] and 'not applied' in lines[0]


def test_fp16_config_restores_mode_on_error(restore_mode):
    _lib.set_math_mode('fp32')
    with pytest.raises(ValueError):
        with config_math_mode(ConfigDict(dict(fp16=dict(loss_scale='dynamic'))), lambda s: None):
            assert _lib.get_math_mode() == 'bf16'
            raise ValueError('training failed')
    assert _lib.get_math_mode() == 'fp32'


def test_config_without_fp16_changes_nothing(restore_mode):
    _lib.set_math_mode('bf16x6')
    cfg = ConfigDict(dict(total_epochs=1))
    assert math_mode_of(cfg) is None
    lines = []
    with config_math_mode(cfg, lines.append) as mode:
        assert mode is None and _lib.get_math_mode() == 'bf16x6'
    assert _lib.get_math_mode() == 'bf16x6' and not lines
