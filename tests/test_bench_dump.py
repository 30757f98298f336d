"""bench.py --dump-outputs (bench.dump_outputs) on a solution rebuilt from a golden region set, so no device is needed: the
files do not depend on the order of the region list, hold the regions' own fields, and a fixed seeded sample keeps them
under the size budget.  And --steps below 1 is refused."""
import os
import random
import subprocess
import sys

import numpy

import bench
from conftest import golden_regions, load_golden, rel_err
from test_export import continuous_solution


def _solution(name):
    sol, _, _ = continuous_solution(name)
    g = golden_regions(load_golden(name))
    for r in sol.critical_regions:
        q = g[tuple(r.active_set)]
        r.omega_set, r.lambda_set, r.regular_set = q['omega_set'], q['lambda_set'], q['regular_set']
    return sol, g


def _load(d):
    return {f[:-4]: numpy.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_order_free_and_holds_the_regions(tmp_path):
    sol, g = _solution('c4_rand_20_8_20_s0')
    random.Random(1).shuffle(sol.critical_regions)
    info = bench.dump_outputs(sol, str(tmp_path / 'a'))
    random.Random(2).shuffle(sol.critical_regions)
    bench.dump_outputs(sol, str(tmp_path / 'b'))
    a, b = _load(tmp_path / 'a'), _load(tmp_path / 'b')
    assert sorted(a) == sorted(b) == sorted(f[:-4] for f in info['files'])
    for name in a:
        assert a[name].dtype == numpy.float64, name
        assert numpy.array_equal(a[name], b[name]), name
    assert info['regions'] == info['regions_in_solution'] == len(g)
    for i, row in enumerate(a['active_set']):
        key = tuple(int(v) for v in row if v >= 0)
        q, k = g[key], len(key)
        r0, r1 = int(a['E_rows'][i]), int(a['E_rows'][i + 1])
        assert rel_err(a['A'][i], q['A']) == 0 and rel_err(a['b'][i], q['b']) == 0
        assert rel_err(a['C'][i][:k], q['C']) == 0 and rel_err(a['d'][i][:k], q['d']) == 0
        assert rel_err(a['E'][r0:r1], q['E']) == 0 and rel_err(a['f'][r0:r1], q['f']) == 0
        assert [int(v) for v in a['omega_set'][i] if v >= 0] == list(q['omega_set'])


def test_dump_samples_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 200_000)
    sol, _ = _solution('c4_rand_20_8_20_s0')
    info = [bench.dump_outputs(sol, str(tmp_path / t)) for t in 'ab']
    assert 0 < info[0]['regions'] < info[0]['regions_in_solution'] and info[0]['bytes'] <= 200_000
    a, b = _load(tmp_path / 'a'), _load(tmp_path / 'b')
    assert all(numpy.array_equal(a[n], b[n]) for n in a)
    assert len(a['region_index']) == len(a['A']) == info[0]['regions']


def test_steps_must_be_at_least_one():
    out = subprocess.run([sys.executable, bench.__file__, '--steps', '0'], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and '--steps must be at least 1' in out.stderr
