"""No-GPU checks of the tap-conv precision switch (gx_tapconv_precision / genesis_amd.set_tapconv_precision): the header declares
the three entry points, the built library exports them, the Python API exists and validates its argument, a fresh process
defaults to mode 0, GENESIS_TAPCONV_PRECISION sets that default, and the switch and gx_matmul_precision leave each other alone.
(Mode switches only set host-side state: nothing here launches a kernel.)"""
import os
import os.path as osp
import re
import subprocess
import sys

import pytest

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith('GENESIS_')}
    env.update(extra)
    return env


def _child(code, **env):
    out = subprocess.run([sys.executable, '-c', code], cwd=REPO, env=_clean_env(**env), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.strip().splitlines()[-1]


def test_header_declares_and_library_exports_the_switch():
    from genesis_amd import _lib
    header = open(osp.join(REPO, 'include', 'genesis_hip.h')).read()
    assert re.search(r'\bint\s+gx_tapconv_precision\s*\(\s*int\s+mode\s*\)\s*;', header)
    assert re.search(r'\bint\s+gx_tapconv_precision_get\s*\(\s*void\s*\)\s*;', header)
    assert re.search(r'\bint\s+gx_tapconv_last_mode\s*\(\s*void\s*\)\s*;', header)
    assert 'GENESIS_TAPCONV_PRECISION' in header
    lib = _lib.load()
    for name in ('gx_tapconv_precision', 'gx_tapconv_precision_get', 'gx_tapconv_last_mode'):
        assert hasattr(lib, name), name


def test_python_api_exists_and_validates():
    import genesis_amd
    assert callable(genesis_amd.set_tapconv_precision) and callable(genesis_amd.get_tapconv_precision)
    before = genesis_amd.get_tapconv_precision()
    for bad in ('high', 'highest', 'low', 3, None, 'MEDIUM '):
        with pytest.raises(ValueError):
            genesis_amd.set_tapconv_precision(bad)
    assert genesis_amd.get_tapconv_precision() == before


def test_fresh_process_defaults_to_mode_0_and_switches():
    code = ('import genesis_amd as g; from genesis_amd import _lib, precision as P; L = _lib.load()\n'
            'r = [g.get_tapconv_precision(), L.gx_tapconv_precision_get(), L.gx_tapconv_last_mode()]\n'
            'g.set_tapconv_precision("medium"); r += [g.get_tapconv_precision(), L.gx_tapconv_precision_get(), P.key()[1]]\n'
            'r.append(L.gx_tapconv_precision(0)); r.append(L.gx_tapconv_precision(3)); r.append(L.gx_tapconv_precision(-1))\n'
            'r.append(g.get_tapconv_precision())\n'
            'r += [L.gx_tapconv_precision(1) < 0, L.gx_tapconv_precision(2) < 0, L.gx_tapconv_precision(-2) < 0]\n'
            'r.append(g.get_tapconv_precision()); r.append(L.gx_tapconv_last_mode())\n'
            'print(r)')
    assert _child(code) == str(['default', 0, -1, 'medium', 3, 3, 3, 0, 3, 'default', True, True, True, 'default', -1])


@pytest.mark.parametrize('value,want', [('medium', 'medium'), ('MEDIUM', 'medium'), ('default', 'default')])
def test_environment_variable_sets_the_default(value, want):
    code = 'import genesis_amd as g; print(g.get_tapconv_precision())'
    assert _child(code, GENESIS_TAPCONV_PRECISION=value) == want
    # -1 goes back to the environment's default
    code = ('import genesis_amd as g; from genesis_amd import _lib\n'
            'g.set_tapconv_precision("default" if %r == "medium" else "medium"); _lib.load().gx_tapconv_precision(-1)\n'
            'print(g.get_tapconv_precision())' % want)
    assert _child(code, GENESIS_TAPCONV_PRECISION=value) == want


def test_unset_environment_variable_changes_nothing():
    code = 'import genesis_amd as g; print((g.get_tapconv_precision(), g.get_matmul_precision()))'
    assert _child(code) == str(('default', 'high'))
    # the matmul level's variable does not reach this switch
    assert _child(code, GENESIS_MATMUL_PRECISION='medium') == str(('default', 'medium'))
    assert _child(code, GENESIS_TAPCONV_PRECISION='medium') == str(('medium', 'high'))


def test_the_two_switches_leave_each_other_alone():
    code = ('import genesis_amd as g; from genesis_amd import _lib, precision as P; L = _lib.load(); r = []\n'
            'for lv in (0, 1, 2, -1): L.gx_matmul_precision(lv); r.append(L.gx_tapconv_precision_get())\n'
            'g.set_tapconv_precision("medium")\n'
            'for lv in (0, 1, 2): L.gx_matmul_precision(lv); r.append(L.gx_tapconv_precision_get())\n'
            'L.gx_matmul_precision(-1); r.append(L.gx_tapconv_precision_get())\n'
            'for lv in ("highest", "medium", "high"):\n'
            '    g.set_matmul_precision(lv)\n'
            '    for m in (0, 3, -1, 3): L.gx_tapconv_precision(m); r.append(g.get_matmul_precision())\n'
            'r.append(P.key()); L.gx_tapconv_precision(0); r.append(P.key()); r.append(P.level())\n'
            'print(r)')
    want = [0, 0, 0, 0, 3, 3, 3, 3] + ['highest'] * 4 + ['medium'] * 4 + ['high'] * 4 + [(1, 3), (1, 0), 1]
    assert _child(code) == str(want)
