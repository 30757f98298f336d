"""bench.py's command line and the record of a plain run, without a device: --full is an option and off by default, the parts of
the full benchmark that have a switch of their own are refused without it, and bench.headline turns a timed region and one
solve's profile into the contract keys."""
import subprocess
import sys
import types

import numpy

import bench


def _run(*argv):
    return subprocess.run([sys.executable, bench.__file__, *argv], capture_output=True, text=True, timeout=120)


def test_full_is_an_option():
    out = _run('--help')
    assert out.returncode == 0 and '--full' in out.stdout


def test_sweep_and_deep_need_full():
    for argv in (['--sweep'], ['--deep', '1']):
        out = _run(*argv)
        assert out.returncode == 2 and 'add --full' in out.stderr, argv


def test_headline_of_a_plain_run():
    prog = types.SimpleNamespace(num_x=lambda: 3, num_t=lambda: 2, num_constraints=lambda: 7, equality_indices=[0], A_t=numpy.zeros((4, 2)))
    prof = [{'depth': 1, 'k': 1, 'candidates': 6, 'status': [0, 1, 2, 3, 0, 0], 'regions': 2},
            {'depth': 2, 'k': 2, 'candidates': 9, 'status': [1, 1, 2, 3, 2, 0], 'regions': 1},
            {'depth': 0, 'k': 1, 'candidates': 1, 'status': [0, 0, 0, 1, 0, 0], 'regions': 1}]
    out = bench.headline('w: a program', prog, 1, False, 4, 2, 0.5, [125.0] * 4, prof, 4)
    assert out['value'] == 16 * 4 / 0.5 and out['ms_per_step'] == 125.0 and out['regions_per_s'] == 4 * 4 / 0.5
    assert (out['unit'], out['higher_is_better'], out['dtype'], out['steps'], out['warmup']) == ('candidates/s', True, 'f64', 4, 2)
    assert out['metric'] == 'candidate active-sets checked/sec (combinatorial mpQP)'
    assert out['config']['candidates_per_step'] == 16 and out['config']['regions_per_step'] == 4 and out['config']['n_tc'] == 4
    assert [lv['candidates'] for lv in out['levels']] == [6, 9]        # the base-set check (depth 0) is no level
    assert 'roofline' not in out and 'cpu_baseline' not in out
