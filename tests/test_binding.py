"""CPU: the ctypes binding takes every prototype from include/nc_hip.h (neuroclear_amd/_lib.py).  The calls below are host arithmetic
or process-wide atomics of the library: none of them needs a GPU."""
import ast
import ctypes
import os
import subprocess

import pytest

from neuroclear_amd import _lib
from neuroclear_amd._lib import I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the functions the binding listed by hand as returning nothing before it read the header
VOID = {'nc_set_force_direct', 'nc_prof_begin', 'nc_sconv_set_cfg', 'nc_sconv_set_tune', 'nc_set_conv_split', 'nc_set_s3_fusion',
        'nc_set_c8x_mode', 'nc_set_split_terms', 'nc_set_h2_guard', 'nc_set_epi_stats', 'nc_set_dl_collapse', 'nc_set_p2d_terms',
        'nc_set_s3x_w64', 'nc_set_unet_lean', 'nc_set_unet_wprep'}


@pytest.fixture(scope='module')
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_one_prototype_per_declared_name():
    protos = _lib.prototypes()
    assert sorted(protos) == _lib.header_symbols()
    assert len(VOID) == 15 and {n for n, (ret, _) in protos.items() if ret is None} == VOID
    # the rule the binding applied to the names before: sizes in bytes or floats (a test export: ..._bytes_debug), and one offset
    by_name = {n for n in protos if n.endswith('_bytes') or n.endswith('_bytes_debug') or n.endswith('_floats') or n == 'nc_h2_cells_offset'}
    assert {n for n, (ret, _) in protos.items() if ret is ctypes.c_size_t} == by_name
    assert [n for n, (ret, _) in protos.items() if ret is ctypes.c_char_p] == ['nc_last_error']
    assert [n for n, (ret, _) in protos.items() if ret is ctypes.c_uint] == ['nc_unet_deconv_kept_expected', 'nc_deep_linear_kept_expected']  # (`kept` words)
    assert all(ret in (ctypes.c_int, ctypes.c_size_t, ctypes.c_uint, ctypes.c_char_p, None) for ret, _ in protos.values())


def test_loaded_library_carries_the_prototypes(L):
    for name, (ret, args) in _lib.prototypes().items():
        fn = getattr(L, name)
        assert fn.restype is ret, name
        assert fn.argtypes is not None and list(fn.argtypes) == args, name
    assert isinstance(L.nc_last_error(), bytes)


@pytest.mark.parametrize('text,names', [('int64_t nc_new_thing(int a);', ('int64_t', 'nc_new_thing')),
                                        ('int nc_new_thing(int a, uint64_t big);', ('uint64_t big', 'nc_new_thing')),
                                        ('int nc_new_thing(unsigned long n);', ('unsigned long n', 'nc_new_thing')),
                                        ('int nc_new_thing(int (*callback)(int));', ('nc_new_thing',))])
def test_unknown_type_raises_and_names_the_declaration(text, names):
    with pytest.raises(_lib.NcError) as e:
        _lib.prototypes('int nc_fine(int a, const float* x);\n' + text)
    for n in names:
        assert n in str(e.value)


def test_plain_and_wrapped_calls_agree(L):
    plain = L.nc_conv_fwd_path(64, 64, 3, 3, 3, 1, 1)
    assert plain == L.nc_conv_fwd_path(I(64), I(64), I(3), I(3), I(3), I(1), I(1))
    assert isinstance(plain, int)
    nb = L.nc_conv_ws_bytes(1, 64, 16, 16, 16, 64, 3, 3, 3, 1, 1)
    assert type(nb) is int and nb == L.nc_conv_ws_bytes(*[I(v) for v in (1, 64, 16, 16, 16, 64, 3, 3, 3, 1, 1)])
    assert type(L.nc_unet_deconv_param_floats()) is int and L.nc_unet_deconv_param_floats() > 0
    od, oh, ow = I(-1), I(-1), I(-1)
    assert L.nc_patchgan_out_shape(4, 1, 36, 36, 3, 64, 2, ctypes.byref(od), ctypes.byref(oh), ctypes.byref(ow)) == 0
    # 4x4 convolutions with padding 1: three of stride 2, then two of stride 1 (36 -> 18 -> 9 -> 4 -> 3 -> 2)
    assert (od.value, oh.value, ow.value) == (1, 2, 2)


@pytest.mark.parametrize('setter,getter', [('nc_set_unet_lean', 'nc_get_unet_lean'), ('nc_set_dl_collapse', 'nc_get_dl_collapse')])
def test_switch_round_trip(L, setter, getter):
    before = getattr(L, getter)()
    try:
        assert getattr(L, setter)(0) is None
        assert getattr(L, getter)() == 0
        getattr(L, setter)(1)
        assert getattr(L, getter)() == 1
    finally:
        getattr(L, setter)(before)
    assert getattr(L, getter)() == before


def test_long_arguments_are_64_bit(L):
    assert L.nc_c8_bytes(1, 8, 1 << 33) == 1 << 37


def test_mistakes_raise_instead_of_running(L):
    with pytest.raises(TypeError):
        L.nc_conv_fwd_path(64, 64, 3, 3, 3, 1)
    with pytest.raises(ctypes.ArgumentError):
        L.nc_conv_fwd_path(64, 64, 3, 3, 3, 1, 1.0)
    with pytest.raises(ctypes.ArgumentError):
        L.nc_c8_bytes(1, 8, I(64))  # a wrapper of another type than the declared one


_WRAPPERS = {'I': ctypes.c_int, 'L_': ctypes.c_long, 'Z': ctypes.c_size_t, 'F': ctypes.c_float, 'CF': ctypes.c_float, 'P': ctypes.c_void_p}


def _wrapper_of(node):
    """The ctypes class an argument expression wraps its value in (I(..), ctypes.c_uint(..), ...), or None."""
    if not isinstance(node, ast.Call):
        return None
    f = node.func
    if isinstance(f, ast.Name):
        return _WRAPPERS.get(f.id)
    if isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and f.value.id == 'ctypes' and f.attr.startswith('c_'):
        return getattr(ctypes, f.attr)
    return None


def _python_sources():
    """Every tracked .py of the repository; without git (an exported tree), every .py below the top level's visible directories."""
    try:
        out = subprocess.run(['git', 'ls-files', '-z', '*.py'], cwd=ROOT, capture_output=True, check=True).stdout.decode()
        paths = [os.path.join(ROOT, f) for f in out.split('\0') if f]
    except (OSError, subprocess.CalledProcessError):
        paths = []
    if not paths:
        for top, dirs, files in os.walk(ROOT):
            dirs[:] = [d for d in dirs if not d.startswith(('.', '_'))]
            paths += [os.path.join(top, f) for f in files if f.endswith('.py')]
    return [p for p in paths if os.path.exists(p) and not os.path.samefile(p, __file__)]  # (this file makes its mistakes on purpose)


def test_every_call_site_matches_the_header():
    """Stands in, on the CPU, for the callers that only run on a GPU: every `<lib>.nc_*(...)` call in the tree passes the declared number
    of arguments, and every argument it wraps explicitly is wrapped in the declared type."""
    protos = _lib.prototypes()
    sites, starred, wrong = 0, 0, []
    for path in _python_sources():
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in protos):
                continue
            sites += 1
            where = '%s:%d %s' % (os.path.relpath(path, ROOT), node.lineno, node.func.attr)
            if any(isinstance(a, ast.Starred) for a in node.args):
                starred += 1
                continue
            argtypes = protos[node.func.attr][1]
            if node.keywords or len(node.args) != len(argtypes):
                wrong.append('%s: %d arguments, %d declared' % (where, len(node.args), len(argtypes)))
                continue
            for i, (a, ty) in enumerate(zip(node.args, argtypes)):
                w = _wrapper_of(a)
                if w is not None and w is not ty:
                    wrong.append('%s: argument %d wrapped as %s, declared %s' % (where, i, w.__name__, ty.__name__))
    print('%d call sites, %d with starred arguments (not checked)' % (sites, starred))
    assert not wrong, '\n'.join(wrong)
    assert sites >= 400
    assert starred <= 0.10 * sites
