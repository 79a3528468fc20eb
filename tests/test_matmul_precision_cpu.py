"""No-GPU checks of the matmul-precision switch: the header declares gx_matmul_precision, the built library exports it, the
per-family modes accept 3, and the Python API (genesis_amd.set_matmul_precision / get_matmul_precision) exists and validates
its argument.  (Mode switches only set host-side state: nothing here launches a kernel.)"""
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
    assert re.search(r'\bint\s+gx_matmul_precision\s*\(\s*int\s+level\s*\)\s*;', header)
    assert re.search(r'\bint\s+gx_matmul_precision_get\s*\(\s*void\s*\)\s*;', header)
    assert 'GENESIS_MATMUL_PRECISION' in header
    lib = _lib.load()
    assert hasattr(lib, 'gx_matmul_precision') and hasattr(lib, 'gx_matmul_precision_get')


def test_python_api_exists_and_validates():
    import genesis_amd
    assert callable(genesis_amd.set_matmul_precision) and callable(genesis_amd.get_matmul_precision)
    with pytest.raises(ValueError):
        genesis_amd.set_matmul_precision('low')
    with pytest.raises(ValueError):
        genesis_amd.set_matmul_precision(2)        # torch's vocabulary only


def test_levels_and_family_modes_in_a_fresh_process():
    code = ('import genesis_amd as g; from genesis_amd import _lib; L = _lib.load(); r = [g.get_matmul_precision()]\n'
            'for lv in ("medium", "highest", "high"): g.set_matmul_precision(lv); r.append(g.get_matmul_precision())\n'
            'r.append(L.gx_matmul_precision(2)); r.append(g.get_matmul_precision())\n'
            'for f in ("kq", "wgq", "wino"): _lib.call("gx_%s_precision" % f, 2)\n'
            'r.append(g.get_matmul_precision()); _lib.call("gx_wino_precision", 3); r.append(g.get_matmul_precision())\n'
            'r.append(L.gx_matmul_precision(-1)); r.append(g.get_matmul_precision()); r.append(L.gx_matmul_precision(3) < 0)\n'
            'print(r)')
    assert _child(code) == str(['high', 'medium', 'highest', 'high', 1, 'medium', 'high', None, 3, 'high', True])


@pytest.mark.parametrize('value,want', [('medium', 'medium'), ('highest', 'highest'), ('high', 'high'), ('HIGH', 'high')])
def test_environment_variable_sets_the_default_ahead_of_the_family_variables(value, want):
    code = 'import genesis_amd as g; print(g.get_matmul_precision())'
    assert _child(code, GENESIS_MATMUL_PRECISION=value, GENESIS_KQ_BF16X6='0', GENESIS_WGQ_F16X3='0') == want
    # set: the level restored by -1 is the environment's
    code = ('import genesis_amd as g; from genesis_amd import _lib; g.set_matmul_precision("highest" if %r != "highest" else "high")\n'
            '_lib.load().gx_matmul_precision(-1); print(g.get_matmul_precision())' % want)
    assert _child(code, GENESIS_MATMUL_PRECISION=value) == want


def test_unset_environment_variable_changes_nothing():
    code = 'import genesis_amd as g; print(g.get_matmul_precision())'
    assert _child(code) == 'high'
    assert _child(code, GENESIS_KQ_F16X3='0') == 'None'          # a per-family variable alone: no common level, as before
