"""ctypes binding of libnc_hip.so.  The prototypes (restype and argtypes of every entry point) are read from include/nc_hip.h,
so a call with a wrong argument count or a float where an int belongs raises instead of running.  The product path has NO
fallback: if the library is missing, or a tensor is not a dense fp32 CUDA(HIP) tensor, the call raises."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# NC_HIP_LIB: load another build of the same library (kernel timing experiments, tools/ablate_*.py)
LIB_PATH = os.environ.get('NC_HIP_LIB') or os.path.join(_HERE, 'csrc', 'libnc_hip.so')
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'nc_hip.h')

_lib = None


class NcError(RuntimeError):
    pass


P = ctypes.c_void_p
I = ctypes.c_int
L_ = ctypes.c_long
F = ctypes.c_float
Z = ctypes.c_size_t

_RET = {'int': I, 'size_t': Z, 'unsigned': ctypes.c_uint, 'void': None, 'const char*': ctypes.c_char_p}
_ARG = {'int': I, 'long': L_, 'size_t': Z, 'unsigned': ctypes.c_uint, 'float': F, 'double': ctypes.c_double}


def prototypes(src=None):
    """{name: (restype, [argtypes])} of every `ret name(params);` in the header text (default: include/nc_hip.h).  Every pointer
    parameter is a c_void_p; a type outside the two tables above raises and names the declaration."""
    if src is None:
        src = open(HEADER_PATH).read()
    src = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', src, flags=re.S)
    src = re.sub(r'^\s*#.*$', '', src, flags=re.M).replace('extern "C" {', '')
    out = {}
    for ret, name, params in re.findall(r'([\w\s\*]+?)\b(nc_\w+)\s*\(([^()]*)\)\s*;', src):
        decl = '%s %s(%s)' % (' '.join(ret.split()), name, ' '.join(params.split()))
        ret = re.sub(r'\s*\*', '*', ' '.join(ret.split()))
        if ret not in _RET:
            raise NcError('nc_hip.h: unknown return type %r in `%s`' % (ret, decl))
        args = []
        for p in ([] if params.strip() in ('', 'void') else params.split(',')):
            if '*' in p or '[' in p:
                args.append(P)
                continue
            words = p.split()
            ty = ' '.join(w for w in (words[:-1] if len(words) > 1 else words) if w != 'const')
            if ty not in _ARG:
                raise NcError('nc_hip.h: unknown parameter type %r in `%s`' % (p.strip(), decl))
            args.append(_ARG[ty])
        if name in out:
            raise NcError('nc_hip.h: `%s` is declared twice' % name)
        out[name] = (_RET[ret], args)
    for name in re.findall(r'\b(nc_\w+)\s*\(', src):
        if name not in out:
            raise NcError('nc_hip.h: cannot parse the declaration of `%s`' % name)
    return out


def header_symbols():
    """Every function name declared in include/nc_hip.h (used by the CPU symbol-export test)."""
    src = open(HEADER_PATH).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(nc_[a-zA-Z0-9_]+)\s*\(', src)))


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NcError('libnc_hip.so is not built (%s): run `python -c "import __graft_entry__ as g; g.build()"` '
                          'or `make -C neuroclear_amd/csrc`; there is no CPU fallback' % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in prototypes().items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def check(code, what=''):
    if code != 0:
        raise NcError('%s failed (%d): %s' % (what, code, lib().nc_last_error().decode()))
