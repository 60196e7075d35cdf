"""CPU: the switch table of the library (csrc/switches.hpp / switches.cpp) built by the host compiler alone with tests/switches_driver.cpp.
Every expectation below is written out from what the code did BEFORE the table existed (each switch's own global, getenv expression and
clamp) -- none is read back from the table -- so a row with a wrong default, clamp or frozen mark fails here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'neuroclear_amd', 'csrc')


def _raw(v): return v
def _bool(v): return int(v != 0)
def _range02(v): return 0 if v < 0 else 2 if v > 2 else v
def _terms(v): return v if v in (0, 3) else 2                  # s3x_set_terms
def _guard(v): return 2 if v == 2 else 1 if v else 0           # h2_guard_set
def _p2d(v): return v if v in (1, 2) else 3                    # p2d_set_terms
def _truth(v): return v != 0                                   # !(getenv(X) && atoi(getenv(X)) == 0): only its truth was ever used


# variable -> (default, how the load-time expression treated the number).  The runtime switches first.
ENV = {
    'NC_CONV_SPLIT': (1, _raw), 'NC_S3_FUSE': (1, _raw), 'NC_SPLIT_TERMS': (2, _raw), 'NC_H2_GUARD': (1, _raw), 'NC_EPI_STATS': (1, _raw),
    'NC_S3X_W64': (1, _raw), 'NC_P2D_TERMS': (1, _raw), 'NC_C8X': (1, _raw),
    'NC_IN_BWD_FOLD': (1, _bool), 'NC_UNET_LEAN': (1, _bool), 'NC_UNET_WPREP': (1, _bool), 'NC_DL_COLLAPSE': (2, _range02),
    # getenv(X) ? atoi(getenv(X)) : default
    'NC_S3X': (1, _raw), 'NC_S3X_WGRAD': (1, _raw), 'NC_HX_WGRAD': (1, _raw), 'NC_S3X_TAIL': (1, _raw), 'NC_S3X_NCB7': (1, _raw),
    'NC_S3X_FLUSH': (4, _raw), 'NC_C1K7_H2': (1, _raw), 'NC_PG1_FEW': (1, _raw), 'NC_P2D': (7, _raw), 'NC_SCONV_CFG': (-1, _raw),
    'NC_H_ABLATE': (0, _raw),
    # !(getenv(X) && atoi(getenv(X)) == 0)
    'NC_C1K3': (1, _truth), 'NC_C1_WGRAD': (1, _truth), 'NC_CONVT_S3X': (1, _truth), 'NC_CONVT_H2': (1, _truth), 'NC_S3_TRAIN_FUSE': (1, _truth),
    'NC_INFER_BATCHED': (1, _truth), 'NC_DL_K32': (1, _truth), 'NC_DL_RANK_WGRAD': (1, _truth), 'NC_DL_RANK_DGRAD': (1, _truth), 'NC_PG1': (1, _truth),
    'NC_SCONV': (1, _truth), 'NC_SCONV_WGRAD': (1, _truth), 'NC_SCONV_TUNE': (1, _truth), 'NC_W_DIFFUSE': (1, _truth),
}
# rows without a variable: identifier -> default (g_force_direct, g_stream_passes, g_k3_on, g_k3_cfg, g_cfg_override, g_tune_mode)
NO_ENV = {'FORCE_DIRECT': 0, 'STREAM_PASSES': 1, 'CONV2D_K3': 1, 'CONV2D_K3_CFG': -1, 'SCONV_CFG_PIN': -1, 'SCONV_TUNE_MODE': -1}
# identifier -> the clamp its setter applied
SETTERS = {
    'FORCE_DIRECT': _raw, 'CONV_SPLIT': _raw, 'S3_FUSE': _raw, 'SPLIT_TERMS': _terms, 'H2_GUARD': _guard, 'IN_BWD_FOLD': _bool, 'STREAM_PASSES': _bool,
    'EPI_STATS': _range02, 'S3X_W64': _bool, 'P2D_TERMS': _p2d, 'C8X': _range02, 'UNET_LEAN': _bool, 'UNET_WPREP': _bool, 'DL_COLLAPSE': _range02,
    'CONV2D_K3': _bool, 'CONV2D_K3_CFG': _raw, 'SCONV_CFG_PIN': _raw, 'SCONV_TUNE_MODE': _raw,
}
FROZEN = {'SPLIT_TERMS', 'H2_GUARD', 'IN_BWD_FOLD', 'STREAM_PASSES'}
# 0, in-range values other than the defaults, out of range on both sides, text that is no number, a number followed by text
TEXTS = ['0', '1', '2', '3', '-1', '-4', '7', 'junk', '5x', '']


def _atoi(text):
    m = re.match(r'\s*([+-]?\d+)', text)
    return int(m.group(1)) if m else 0


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++')) if c), None)
    if cxx is None:
        pytest.skip('no C++ compiler available')
    exe = str(tmp_path_factory.mktemp('switches') / 'switches_driver')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-pthread', os.path.join(ROOT, 'tests', 'switches_driver.cpp'),
                    os.path.join(CSRC, 'switches.cpp'), '-o', exe], check=True, capture_output=True)

    def run(mode, env=None):
        clean = {k: v for k, v in os.environ.items() if not k.startswith('NC_')}
        clean.update(env or {})
        r = subprocess.run([exe, mode], env=clean, capture_output=True, text=True)
        return r.returncode, [line.split() for line in r.stdout.splitlines()]
    return run


def _rows(driver, env=None):
    code, lines = driver('rows', env)
    assert code == 0 and lines and all(f[0] == 'ROW' and len(f) == 5 for f in lines), lines
    return {f[1]: (f[2], int(f[3]), int(f[4])) for f in lines}  # identifier -> (variable, frozen, value)


def test_rows_are_the_switches_the_code_had(driver):
    rows = _rows(driver)
    assert sorted(v[0] for v in rows.values() if v[0] != '-') == sorted(ENV), 'one row per variable, no variable twice'
    assert {i for i, v in rows.items() if v[0] == '-'} == set(NO_ENV)
    assert {i for i, v in rows.items() if v[1]} == FROZEN
    assert set(SETTERS) <= set(rows)
    for ident, (var, _, _) in rows.items():
        if var != '-':
            assert var == 'NC_' + ident, (ident, var)


def test_defaults_in_a_clean_environment(driver):
    for ident, (var, _, value) in _rows(driver).items():
        want = NO_ENV[ident] if var == '-' else ENV[var][0]
        print(ident, value, want)
        assert value == want, ident


@pytest.mark.parametrize('text', TEXTS)
def test_every_variable_parses_as_before(driver, text):
    rows = _rows(driver, {var: text for var in ENV})
    for ident, (var, _, value) in rows.items():
        if var == '-':
            assert value == NO_ENV[ident], ident
            continue
        want = ENV[var][1](_atoi(text))
        print(var, repr(text), value, want)
        if ENV[var][1] is _truth:
            assert (value != 0) == want, (var, text)
        else:
            assert value == want, (var, text)


def test_documented_discrepancies_between_variable_and_setter(driver):
    """Kept as they were, not unified: the load-time read of these stores the number as given, the setter clamps."""
    rows = _rows(driver, {'NC_SPLIT_TERMS': '5', 'NC_DL_COLLAPSE': '7', 'NC_H2_GUARD': '7', 'NC_EPI_STATS': '-1'})
    assert rows['SPLIT_TERMS'][2] == 5 and rows['DL_COLLAPSE'][2] == 2 and rows['H2_GUARD'][2] == 7 and rows['EPI_STATS'][2] == -1
    assert _rows(driver, {'NC_DL_COLLAPSE': '-1'})['DL_COLLAPSE'][2] == 0
    assert SETTERS['SPLIT_TERMS'](5) == 2 and SETTERS['H2_GUARD'](7) == 1 and SETTERS['EPI_STATS'](-1) == 0


def test_setters_clamp_and_return_the_previous_value(driver):
    code, lines = driver('set')
    assert code == 0
    now = {i: v[2] for i, v in _rows(driver).items()}
    seen = set()
    for tag, ident, arg, prev, after in lines:
        assert tag == 'SET'
        arg, prev, after = int(arg), int(prev), int(after)
        assert prev == now[ident], (ident, arg)
        want = SETTERS.get(ident, _raw)(arg)
        assert after == want, (ident, arg, after, want)
        now[ident] = after
        seen.add((ident, arg))
    assert seen == {(i, a) for i in now for a in (-3, -1, 0, 1, 2, 3, 5, 7)}


def test_scope_rules(driver):
    code, lines = driver('scope')
    print('\n'.join(' '.join(f) for f in lines))
    names = [f[1] for f in lines]
    assert len(lines) >= 45 and all(f[0] == 'CHECK' for f in lines) and len(set(names)) == len(names)
    for tag in ('switch_scope', 'network_scope'):
        for what in ('keeps_frozen_rows', 'raw_moves', 'other_rows_live', 'is_per_thread', 'closed_sees_now', 'closed_all_clear'):
            assert '%s_%s' % (tag, what) in names
    for must in ('nested_outer_close_clears', 'force2_outside_restores', 'force2_inside_restores_sample', 'force2_inside_scope_close_clears',
                 'force3_nested_close_still_on', 'force3_closed_off'):
        assert must in names
    for m in range(3):
        for where in ('outside', 'switch_scope', 'network_scope', 'network_scope_after_inner', 'outside_again'):
            assert 'can_flip_mode%d_%s' % (m, where) in names
    assert [f for f in lines if f[2] != 'ok'] == [] and code == 0


def test_integration_md_lists_every_variable(driver):
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    listed = re.findall(r'^\s*\| `(NC_[A-Z0-9_]+)` \|', text, flags=re.M)
    in_table = sorted(v[0] for v in _rows(driver).values() if v[0] != '-')
    assert sorted(listed) == in_table


def test_one_getenv_in_the_library():
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(('.hip', '.hpp', '.cpp', '.h')):
            for n, line in enumerate(open(os.path.join(CSRC, name)), 1):
                code = line.split('//')[0]
                if 'getenv(' in code:
                    hits.append('%s:%d' % (name, n))
                assert 'frozen_' not in code and 'tl_sw_' not in code, '%s:%d' % (name, n)
    assert len(hits) == 1 and hits[0].startswith('switches.cpp:'), hits
