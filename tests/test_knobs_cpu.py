"""The library's environment knobs (ppopt_amd/csrc/knobs.hpp): one table, one parser.  A tiny C++ program that includes the header
alone (g++, no HIP) prints every knob for a given environment; the expected values are written here from the parse rules, kind by
kind, not taken from the program.  The table is also compared with the documented one and with the
variable names that appear as strings in the header."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, 'ppopt_amd', 'csrc', 'knobs.hpp')

MAIN = r'''
#include "knobs.hpp"
#include <cstdio>
#include <cstring>
using namespace mpc;
static const char *when_name(KnobWhen w) { return w == KnobWhen::handle ? "handle" : (w == KnobWhen::process ? "process" : "call"); }
static void print_value(const KnobRow &r, const Knobs &k) {
    if (r.pi) std::printf("%s=%d\n", r.name, k.*r.pi);
    else if (r.pb) std::printf("%s=%d\n", r.name, (int)(k.*r.pb));
    else if (r.pl) std::printf("%s=%lld\n", r.name, k.*r.pl);
    else if (r.pd) std::printf("%s=%.17g\n", r.name, k.*r.pd);
    else std::printf("%s=%.17g\n", r.name, knob_process(r.name));
}
int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--list") == 0) {
        const Knobs k;   // the defaults
        for (const KnobRow &r : KNOB_TABLE) {
            if (r.when == KnobWhen::handle) { std::printf("%s ", when_name(r.when)); print_value(r, k); }
            else std::printf("%s %s=%.17g\n", when_name(r.when), r.name, r.dflt);
        }
        return 0;
    }
    const Knobs k = Knobs::from_env();
    for (const KnobRow &r : KNOB_TABLE) print_value(r, k);
    return 0;
}
'''

# name -> (kind, default), from the rules of the table in the header's documentation: per handle ...
FLAG = ['FORCE_V1', 'DEBUG_CYCLES', 'NO_RSPLIT', 'NO_RBOX', 'NO_ROVERLAP', 'NO_KKT_LISTS', 'NO_SMALL_RX', 'NO_SMALL_FUSE', 'NO_SMALLPATH',
        'TEST_SMALL_FALLBACK', 'NO_EQ_ELIM', 'KKT_BOX_SELECT']
KNOBS = {f'MPC_{n}': ('flag', 0) for n in FLAG}
KNOBS['MPC_DEBUG_CREATE'] = ('present', 0)
KNOBS.update({f'MPC_{n}': ('int', d) for n, d in (('X1_DEFER', 1), ('KKT_SPREAD', 1), ('XQ_THREAD', -1), ('X1', 2), ('NO_KKT_THREAD', 0),
                                                  ('TEST_LATE', 0), ('TEST_SPARE', 0), ('TH_DIV', 4), ('TH_MAXW', 2))})
KNOBS.update({f'MPC_{n}': ('int_ge0', d) for n, d in (('KKT_SPREAD_THREADS', 1 << 19), ('X_SECOND_MAX', 1024), ('XQ_SKIP_BELOW', 100000))})
KNOBS.update({f'MPC_{n}': ('int_gt0', d) for n, d in (('XQT_WPC', 16), ('X1_WPC', 16), ('X2_WPC', 12), ('XQ_WPC', 20), ('XQG_PER_CU', 4), ('X2_DIV', 16))})
KNOBS['MPC_R2_CAP'] = ('pct_gt0', 100)
KNOBS.update({f'MPC_{n}': ('int64', d) for n, d in (('PRUNED_BUCKET_NP', 1024), ('XQT_MIN', 4096), ('X1_MIN', 2048), ('XQ_EARLY_REGIONS', 0),
                                                    ('X_FIRST_MIN', 4096), ('X_FIRST_MAX', 65536), ('SMALLPATH_MAX', 4096), ('ROVERLAP_MIN', 2048),
                                                    ('ROVERLAP_LONG', 50000))})
KNOBS.update({f'MPC_{n}': ('double', d) for n, d in (('X_FRESH_LIMIT', 1e6), ('PRUNED_BUCKET_MIN', 2e7), ('DICT_BUDGET_GB', 48.0))})
KNOBS['MPC_RSPLIT_MAX'] = ('rsplit', 4)
HANDLE = set(KNOBS)
# ... and process-wide (read once per process, MPC_BATCH_BUDGET_GB at every call)
KNOBS.update({'MPC_DEV_POOL_GB': ('double', 48.0), 'MPC_BATCH_BUDGET_GB': ('double', 160.0), 'MPC_DEBUG_MANY': ('flag', 0), 'MPC_DEBUG_SMALL': ('flag', 0)})
KNOBS.update({f'MPC_BATCH_{n}': ('int_nonempty', d) for n, d in (('WPC_TH', 32), ('WPC_XQ', 20), ('WPC_X2', 12), ('WPC_R2', 16), ('SHARES', 1), ('WSHARE', 1))})
WHEN = {n: 'handle' if n in HANDLE else ('call' if n == 'MPC_BATCH_BUDGET_GB' else 'process') for n in KNOBS}


def c_atoi(s):
    m = re.match(r'\s*([+-]?\d+)', s)
    return int(m.group(1)) if m else 0


def c_atof(s):
    m = re.match(r'\s*([+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?)', s)
    return float(m.group(1)) if m else 0.0


def expected(kind, default, s):
    """s: the variable's text, None when it is unset"""
    if kind == 'flag':
        return int(s is not None and s[:1] == '1')
    if kind == 'present':
        return int(s is not None)
    if s is None:
        return default
    v = c_atoi(s)
    return {'int': v, 'int_ge0': max(0, v), 'int_gt0': v if v > 0 else default, 'pct_gt0': min(100, v) if v > 0 else default, 'int64': v,
            'double': c_atof(s), 'rsplit': 16 if v >= 16 else 8 if v >= 8 else 4 if v >= 4 else 2 if v >= 2 else 1,
            'int_nonempty': v if s != '' else default}[kind]


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ is needed to build the knob printer')
    tmp = tmp_path_factory.mktemp('knobs')
    src, exe = str(tmp / 'main.cpp'), str(tmp / 'knobs')
    open(src, 'w').write(MAIN)
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-I', os.path.dirname(HEADER), src, '-o', exe])
    return exe


def run(exe, env, *args):
    base = {k: v for k, v in os.environ.items() if not k.startswith('MPC_')}
    out = subprocess.check_output([exe, *args], env={**base, **env}).decode()
    return [line for line in out.split('\n') if line]


def values(exe, env):
    got = dict(line.split('=', 1) for line in run(exe, env))
    assert set(got) == set(KNOBS)
    return {k: float(v) for k, v in got.items()}


@pytest.mark.parametrize('text', [None, '1', '0', '', '10', '01', '-3', 'abc', '2.5e3'])
def test_every_knob_parses_by_its_kind(program, text):
    """every variable at once set to `text` (None: unset, which gives the defaults)"""
    got = values(program, {} if text is None else {name: text for name in KNOBS})
    for name, (kind, default) in KNOBS.items():
        assert got[name] == expected(kind, default, text), (name, kind, text)


def test_one_knob_set_leaves_the_others_at_their_defaults(program):
    for name in ('MPC_X1_MIN', 'MPC_NO_RBOX', 'MPC_BATCH_WSHARE', 'MPC_DICT_BUDGET_GB'):
        got = values(program, {name: '7'})
        for other, (kind, default) in KNOBS.items():
            assert got[other] == (expected(kind, default, '7') if other == name else default), (name, other)


@pytest.mark.parametrize('text,want', [('0', 1), ('1', 1), ('3', 2), ('4', 4), ('7', 4), ('8', 8), ('100', 16)])
def test_rsplit_max_rounds_down_to_a_power_of_two(program, text, want):
    assert values(program, {'MPC_RSPLIT_MAX': text})['MPC_RSPLIT_MAX'] == want


def test_special_cases(program):
    assert values(program, {'MPC_R2_CAP': '250'})['MPC_R2_CAP'] == 100
    assert values(program, {})['MPC_X1'] == 2                    # the effective default, not the old member initialiser
    assert values(program, {'MPC_DEBUG_CREATE': ''})['MPC_DEBUG_CREATE'] == 1
    assert values(program, {'MPC_BATCH_WPC_TH': ''})['MPC_BATCH_WPC_TH'] == 32   # empty counts as unset for the shares only
    assert values(program, {'MPC_X1': ''})['MPC_X1'] == 0


def documented():
    """rows of the library's table in INTEGRATION.md section 5: name -> (default, read when)"""
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    section = text[text.index('## 5. Environment knobs'):text.index('### 5.1')]
    rows = {}
    for m in re.finditer(r'^\| `(MPC_[A-Z0-9_]+)` \| ([^|]+) \| per (handle|process|call) \|', section, flags=re.M):
        rows[m.group(1)] = (float(m.group(2)), m.group(3))
    return rows


def test_table_matches_documentation_and_header(program):
    listed = {}
    for line in run(program, {}, '--list'):
        when, rest = line.split(' ', 1)
        name, default = rest.split('=', 1)
        listed[name] = (float(default), when)
    assert listed == {name: (float(default), WHEN[name]) for name, (_, default) in KNOBS.items()}
    assert documented() == listed
    strings = set(re.findall(r'"(MPC_[A-Z0-9_]+)"', open(HEADER).read()))
    assert strings == set(listed)


def test_getenv_only_in_the_knob_header():
    csrc = os.path.dirname(HEADER)
    users = [f for f in sorted(os.listdir(csrc)) if f.endswith(('.hip', '.hpp')) and 'getenv' in open(os.path.join(csrc, f)).read()]
    assert users == ['knobs.hpp']
