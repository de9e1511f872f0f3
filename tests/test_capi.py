"""The C-ABI library loads and exports every symbol include/lsnet_hip.h declares, with the signatures and the struct
layouts the header gives them (no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

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


def _header_text():
    text = open(os.path.join(ROOT, 'include', 'lsnet_hip.h')).read()
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def _prototypes():
    """[(return type, name, [(parameter type, parameter name)])] of every function the header declares, types normalised
    to single spaces with `const` dropped and the stars attached ('float*')."""
    def norm(t):
        return re.sub(r'\s*\*', '*', ' '.join(re.sub(r'\bconst\b', ' ', t).split()))
    out = []
    for ret, name, params in re.findall(r'^\s*((?:const\s+)?[A-Za-z_][\w ]*?[\s\*]+)(lsn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;',
                                        _header_text(), flags=re.M):
        plist = []
        if params.strip() != 'void':
            for p in params.split(','):
                m = re.fullmatch(r'(.*?)(\w+)', p.strip(), flags=re.S)
                plist.append((norm(m.group(1)), m.group(2)))
        out.append((norm(ret), name, plist))
    return out


_SCALARS = {'int': ctypes.c_int, 'lsn_layout': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float,
            'double': ctypes.c_double, 'lsn_stream_t': ctypes.c_void_p}
_POINTEES = ('float', 'void', 'int', 'int32_t', 'int64_t', 'uint8_t', 'long long')
_RETURNS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'char*': ctypes.c_char_p}


def test_signatures_match_header(built_lib):
    """restype and argtypes of every function of the loaded library are what the header's prototype maps to: scalars
    exactly, pointers to scalars / void as c_void_p, a struct pointer as POINTER(its mirror) or c_void_p."""
    from lsnet_amd import _lib
    lib = _lib.load()
    protos = _prototypes()
    assert len(protos) >= 99
    assert [name for _, name, _ in protos] == list(_lib.EXPORTS)      # the same names, in header order
    for ret, name, params in protos:
        fn = getattr(lib, name)
        assert fn.restype is _RETURNS[ret], (name, ret, fn.restype)
        assert fn.argtypes is not None, f'{name} has no argtypes'
        assert len(fn.argtypes) == len(params), (name, len(fn.argtypes), len(params))
        for i, ((ctype, pname), got) in enumerate(zip(params, fn.argtypes)):
            where = f'{name} argument {i} ({ctype} {pname})'
            if ctype in _SCALARS:
                assert got is _SCALARS[ctype], (where, got)
            elif ctype.endswith('*') and ctype[:-1] in _POINTEES:
                assert got is ctypes.c_void_p, (where, got)
            else:
                assert re.fullmatch(r'lsn_\w+\*', ctype), where
                assert got is ctypes.c_void_p or (issubclass(got, ctypes._Pointer) and got._type_.c_name == ctype[:-1]), (where, got)


def test_struct_layouts_match_compiler(tmp_path):
    """Size of every struct mirror, offset and size of every field, against what the host compiler lays out for the
    header's typedef of that name; and every struct typedef of the header has a mirror."""
    from lsnet_amd import _lib
    typedefs = set(re.findall(r'\}\s*(lsn_\w+)\s*;', _header_text())) - {'lsn_status', 'lsn_layout'}
    assert typedefs == {m.c_name for m in _lib.STRUCTS} and len(typedefs) == len(_lib.STRUCTS) >= 16
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "lsnet_hip.h"', 'int main(void) {']
    for m in _lib.STRUCTS:
        lines.append(f'    printf("{m.c_name} %zu\\n", sizeof({m.c_name}));')
        for field, _ in m._fields_:
            lines.append(f'    printf("{m.c_name}.{field} %zu %zu\\n", offsetof({m.c_name}, {field}), '
                         f'sizeof((({m.c_name} *)0)->{field}));')
    lines += ['    return 0;', '}', '']
    src, exe = tmp_path / 'layout.cpp', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'no host compiler'
    r = subprocess.run([cxx, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr       # (a mirror field the header does not have ends here)
    compiled = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        key, *nums = line.split()
        compiled[key] = tuple(int(v) for v in nums)
    for m in _lib.STRUCTS:
        assert compiled[m.c_name] == (ctypes.sizeof(m),), (m.c_name, compiled[m.c_name], ctypes.sizeof(m))
        for field, _ in m._fields_:
            d = getattr(m, field)
            assert compiled[f'{m.c_name}.{field}'] == (d.offset, d.size), (m.c_name, field, compiled[f'{m.c_name}.{field}'],
                                                                          (d.offset, d.size))


def test_wide_ints_survive(built_lib):
    """Every scalar int64_t parameter of the header is declared c_int64 to ctypes: a value above 2^31 reaches the callee
    whole, without a wrapper at the call site."""
    from lsnet_amd import _lib
    lib = _lib.load()
    wide = [(name, i) for _, name, params in _prototypes() for i, (ctype, _) in enumerate(params) if ctype == 'int64_t']
    assert len(wide) >= 8
    for name, i in wide:
        assert getattr(lib, name).argtypes[i] is ctypes.c_int64, (name, i)
    # what the declaration guarantees, through ctypes' own conversion of a typed call (from_param returns an opaque
    # argument object for a plain int, so the value is read back from a callee)
    echo = ctypes.CFUNCTYPE(ctypes.c_int64, ctypes.c_int64)(lambda v: v)
    assert echo(2**33 + 5) == 2**33 + 5


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
