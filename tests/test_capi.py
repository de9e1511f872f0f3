"""The C-ABI library loads and exports every symbol include/lsnet_hip.h declares (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built_lib():
    from lsnet_amd.csrc import build
    return build.build()


def _declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'lsnet_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(lsn_[a-z0-9_]+)\s*\(', text)))


def test_header_symbols_are_exported(built_lib):
    lib = ctypes.CDLL(built_lib)
    names = _declared_symbols()
    assert len(names) >= 19
    for n in names:
        assert hasattr(lib, n), f'{n} declared in lsnet_hip.h but not exported'


def test_loader_export_list_matches_header(built_lib):
    from lsnet_amd import _lib
    assert sorted(_lib.EXPORTS) == _declared_symbols()
    lib = _lib.load()
    assert lib.lsn_version() >= 100
    assert isinstance(lib.lsn_last_error(), bytes)


def test_argument_checks_need_no_gpu(built_lib):
    """Shape validation happens before any device work (mirrors the reference's TORCH_CHECKs)."""
    from lsnet_amd import _lib
    lib = _lib.load()
    # kernel size 0 -> LSN_ERR_INVALID with the reference's message
    rc = lib.lsn_deform_conv_forward(None, None, None, None, 1, 4, 8, 8, 4, 0, 0, 1, 1, 0, 0, 1, 1, 1, 1, 1, None)
    assert rc == -1 and b'kernel size should be greater than zero' in lib.lsn_last_error()
    # input smaller than kernel (deform_conv_cuda.cpp:128)
    rc = lib.lsn_deform_conv_forward(None, None, None, None, 1, 4, 2, 2, 4, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, None)
    assert rc == -1 and b'input image is smaller than kernel' in lib.lsn_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(rc)


def _debug_bits():
    """{name: value} of the LSN_DBG_* enum of include/lsnet_hip.h, without the prefix LSN_"""
    text = open(os.path.join(ROOT, 'include', 'lsnet_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    bits = {}
    for name, value in re.findall(r'\bLSN_(DBG_[A-Z0-9_]+)\s*=\s*([^,}]+)', text):
        shift = re.fullmatch(r'1\s*<<\s*(\d+)', value.strip())
        bits[name] = 1 << int(shift.group(1)) if shift else int(value, 0)
    return bits


def test_debug_word_constants_match_header():
    from lsnet_amd import _lib
    bits = _debug_bits()
    assert len(bits) == 8 and bits['DBG_BLOCK_MASK'] == 0xffff
    for name, value in bits.items():
        assert getattr(_lib, name) == value, name


def test_debug_word_refuses_unknown_bits(built_lib):
    """lsn_debug_phase_clocks takes a workgroup index and the named routing bits.  Any other bit is refused: the bits of
    finished experiments (17, 26, 27, 29, 30), the old places of the moved ones (16, 18, 19) and bits that never meant
    anything.  The _lib setter raises for the same words."""
    from lsnet_amd import _lib
    lib = _lib.load()
    bits = _debug_bits()
    named = [v for k, v in bits.items() if k != 'DBG_BLOCK_MASK']
    known = bits['DBG_BLOCK_MASK'] | sum(named)
    unknown = [1 << b for b in range(32) if not (known >> b) & 1]
    assert {1 << b for b in (16, 17, 18, 19, 26, 27, 29, 30, 31)} == set(unknown)
    try:
        for word in unknown + [(1 << 26) | 5, (1 << 27) | _lib.DBG_GENERAL_GEMMS]:
            assert lib.lsn_debug_phase_clocks(None, ctypes.c_int(word)) == -1, hex(word)
            assert b'unknown debug bits' in lib.lsn_last_error()
            with pytest.raises(RuntimeError, match='unknown debug bits'):
                _lib.set_debug_word(word)
        for word in [0, 300, bits['DBG_BLOCK_MASK']] + named + [sum(named) | 17]:
            assert lib.lsn_debug_phase_clocks(None, ctypes.c_int(word)) == 0, hex(word)
            _lib.set_debug_word(word)
    finally:
        _lib.set_debug_word(0)


def test_product_ops_refuse_cpu_tensors():
    """No CPU fallback in the product: like the reference (deform_conv.py:46-47) CPU tensors raise in the device-only ops."""
    import torch
    from lsnet_amd import ops
    x = torch.zeros(1, 4, 5, 5)
    with pytest.raises(NotImplementedError):
        ops.deform_conv(x, torch.zeros(1, 18, 5, 5), torch.zeros(4, 4, 3, 3), padding=1)
    with pytest.raises(NotImplementedError):
        ops.sigmoid_focal_loss(torch.zeros(4, 3), torch.zeros(4, dtype=torch.long))
    # NMS is the one op the reference itself serves on the host (nms_wrapper.py:33-37 -> nms_cpu): CPU tensors take the
    # host library's counterpart, they never reach (or replace) the device kernel
    dets, keep = ops.nms(torch.tensor([[0., 0., 2., 2., .9], [0., 0., 2., 2., .8], [5., 5., 6., 6., .7]]), 0.5)
    assert keep.tolist() == [0, 2] and dets.shape == (2, 5)
