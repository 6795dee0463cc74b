"""bench.py's legs: a plain run measures the headline alone (set-up, warm-up, the timed steps, the result line); --full adds the roofline,
the whole-games leg, the secondary leg and the CPU baseline.  Small sizes: what is checked is which legs run, not their figures."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ('roofline', 'roofline_net', 'sustained', 'value_whole_games', 'secondary', 'cpu_baseline')


def run_bench(*args):
    env = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'AZG_BENCH_SPAWN', 'AZG_FORCE_DIST'):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--games', '64', '--sims', '32', '--steps', '6', '--warmup', '1'] + list(args)
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r['unit'] == 'env-steps/sec' and r['higher_is_better'] is True and r['dtype'] == 'f64'
    assert r['value'] > 0 and r['engine_errors'] == 0 and r['steps'] == 6 and r['warmup'] == 1
    assert abs(r['value'] * r['ms_per_step'] * r['steps'] / 1e3 - r['plies_completed']) < 1.0
    return r


def test_bench_plain_run_is_the_headline_alone():
    r = run_bench()
    assert not [k for k in EXTRAS if k in r], [k for k in EXTRAS if k in r]


def test_bench_full_run_has_every_leg():
    r = run_bench('--full', '--roofline-rounds', '64', '--sustained-steps', '2', '--cpu-procs', '1', '--cpu-seconds', '1')
    assert r['roofline']['select_ms'] > 0 and r['roofline_net']['achieved'] > 0
    assert r['sustained']['value'] > 0 and r['value_whole_games'] == r['sustained']['value'] and r['sustained']['engine_errors'] == 0
    assert r['secondary']['value'] > 0 and r['secondary']['engine_errors'] == 0 and r['secondary']['roofline']
    assert r['cpu_baseline']['value'] > 0 and r['secondary']['cpu_baseline']['value'] > 0
