"""The GENESIS_* environment variables: INTEGRATION.md section 4 lists exactly the ones the tree reads, and the package reads at
most 40 of them (VERDICT.md, item 8 of "Next round").  Plain text scans: no GPU, no build."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = re.compile(r'GENESIS_[A-Z0-9_]+')
NOT_VARIABLES = {'GENESIS_HIP_H'}          # the include guard of include/genesis_hip.h


def _table():
    """{variable: 'read by' cell} from the table "Environment variables" of INTEGRATION.md."""
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    section = text.split('## 4. Environment variables', 1)[1]
    rows = {}
    for line in section.splitlines():
        cells = [c.strip() for c in line.strip().strip('|').split('|')]
        m = re.fullmatch(r'`(GENESIS_[A-Z0-9_]+)`', cells[0]) if len(cells) == 4 else None
        if m:
            assert m.group(1) not in rows, 'listed twice: ' + m.group(1)
            rows[m.group(1)] = cells[3]
    assert rows, 'no table under "## 4. Environment variables"'
    return rows


def _names_in(paths):
    found = {}
    for p in paths:
        with open(os.path.join(ROOT, p), errors='replace') as f:
            for n in NAME.findall(f.read()):
                found.setdefault(n, p)
    return found


def _package_sources():
    out = []
    for d, _, files in os.walk(os.path.join(ROOT, 'genesis_amd')):
        out += [os.path.relpath(os.path.join(d, f), ROOT) for f in files if f.endswith(('.py', '.hip', '.cpp', '.h'))]
    return out


def test_package_variables_are_the_table():
    table = _table()
    in_source = _names_in(_package_sources())
    missing = {n: p for n, p in in_source.items() if n not in table}
    assert not missing, 'named under genesis_amd/ but not in INTEGRATION.md section 4: %s' % missing
    package_rows = {n for n, where in table.items() if 'genesis_amd/' in where}
    stale = sorted(package_rows - set(in_source))
    assert not stale, 'listed as read by the package but named nowhere under genesis_amd/: %s' % stale


def test_at_most_forty_package_variables():
    names = sorted(_names_in(_package_sources()))
    assert len(names) <= 40, (len(names), names)


def test_no_tracked_source_names_an_unlisted_variable():
    try:
        tracked = subprocess.run(['git', 'ls-files'], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True,
                                 universal_newlines=True).stdout.split('\n')
    except (OSError, subprocess.CalledProcessError):          # (an exported tree: every file under it)
        tracked = [os.path.relpath(os.path.join(d, f), ROOT) for d, _, files in os.walk(ROOT) for f in files
                   if '.git' not in d.split(os.sep)]
    sources = [p for p in tracked if p.endswith(('.py', '.sh', '.hip', '.cpp', '.h')) and os.path.isfile(os.path.join(ROOT, p))]
    assert len(sources) > 50, sources
    table = _table()
    unknown = {n: p for n, p in _names_in(sources).items() if n not in table and n not in NOT_VARIABLES}
    assert not unknown, 'not in INTEGRATION.md section 4: %s' % unknown
