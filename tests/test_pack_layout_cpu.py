"""The packed-weight descriptor (genesis_amd/csrc/gx_pack.h) on the host: tests/pack_layout_main.cpp packs random weights
with the functions the pack kernels use and checks every (view, form) for overlapping words, words outside the packing's
size, the trailer's place, the decoded values against the source weights, and the validity table.  No GPU."""
import os
import os.path as osp
import shutil
import subprocess

import pytest

HERE = osp.dirname(osp.abspath(__file__))
CSRC = osp.join(osp.dirname(HERE), 'genesis_amd', 'csrc')


def _hipcc():
    cand = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    return cand if osp.exists(cand) else shutil.which('hipcc')


def test_pack_layout_host_program(tmp_path):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip('hipcc is not installed: the host layout program cannot be compiled')
    exe = str(tmp_path / 'pack_layout')
    cc = subprocess.run([hipcc, '-x', 'hip', '--offload-host-only', '-O2', '-std=c++17', '-I' + CSRC,
                         osp.join(HERE, 'pack_layout_main.cpp'), '-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert cc.returncode == 0, cc.stdout.decode()
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = run.stdout.decode()
    print(out)
    assert run.returncode == 0, out
    last = out.strip().splitlines()[-1]
    assert last.startswith('pack layout: ') and last.endswith(' 0 failures'), out
    assert int(last.split()[2]) >= 48 * 8, out      # every valid pair at every channel pair
