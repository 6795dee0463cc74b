"""CPU-only: the surface of the one-ply lookahead and the greedy contestants -- azg_env_lookahead and azg_greedy_candidates declared in
include/azg.h, exported by the built library and bound by _lib.py; HipGame.lookahead_batch, games.greedy_candidates,
arena.GreedyContestant and arena.vs_greedy with their signatures; the new translation unit in build.py with the playout unit's flags."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'alpha-zero-general_amd', 'libazg_hip.so')

DECLARED = {
    'azg_env_lookahead': ['game', 'variant', 'states_dev', 'players_dev', 'active_dev', 'n', 'waves_per_state', 'rng_seed', 'stream0',
                          'counters_dev', 'out_valid_dev', 'out_scores_dev', 'out_ended_dev', 'out_next_player_dev', 'out_states_dev', 'stream'],
    'azg_greedy_candidates': ['game', 'variant', 'rule', 'canonical_states_dev', 'valid_dev', 'scores_dev', 'n', 'active_dev',
                              'out_candidates_dev', 'stream'],
}


def signature(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_entry_points_are_declared_exported_and_bound():
    from azg_amd import _lib
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'azg.h')).read(), flags=re.S)
    for name, names in DECLARED.items():
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, h)
        assert m, 'include/azg.h does not declare %s' % name
        params = [' '.join(p.split()) for p in m.group(1).split(',')]
        assert [p.split()[-1].lstrip('*') for p in params] == names, params
        assert name in _lib.EXPORTS
        assert hasattr(ctypes.CDLL(LIB), name)
        assert len(getattr(_lib.lib(), name).argtypes) == len(names)
    assert re.search(r'#define\s+AZG_GREEDY_REFERENCE\s+0\b', h) and re.search(r'#define\s+AZG_GREEDY_LEAD\s+1\b', h)
    assert 'const uint64_t* counters_dev' in re.search(r'\bint\s+azg_env_lookahead\s*\(([^;]*)\)', h).group(1)     # never written


def test_python_surface():
    from azg_amd import arena, games
    empty = inspect.Parameter.empty
    assert signature(games.HipGame.lookahead_batch) == [
        ('self', empty), ('boards', empty), ('players', None), ('active', None), ('waves_per_state', None), ('stream0', 0), ('counters', None),
        ('successor_states', False)]
    assert games.Lookahead._fields == ('valid', 'scores', 'ended', 'next_player', 'states')
    assert games.GREEDY_RULES == {'reference': 0, 'lead': 1}
    assert signature(games.greedy_candidates) == [('game', empty), ('rule', empty), ('canonical', empty), ('valid', empty), ('scores', empty),
                                                  ('active', None), ('out', None)]
    assert signature(arena.GreedyContestant.__init__) == [('self', empty), ('rule', 'reference')]
    assert arena.GreedyContestant.mode == arena.RandomContestant.mode == arena.PICK_UNIFORM
    assert signature(arena.GreedyContestant.probs_valid) == signature(arena.RandomContestant.probs_valid)
    assert signature(arena.vs_greedy) == [('game', empty), ('nnet', empty), ('args', empty), ('num', empty), ('rule', 'reference'), ('kw', empty)]
    for bad in ('Reference', 'greedy', None, 0):
        try:
            arena.GreedyContestant(bad)
        except ValueError:
            continue
        raise AssertionError('GreedyContestant(%r) was accepted' % (bad,))


def test_default_waves_per_state_is_a_rule_on_the_action_count():
    from azg_amd import games
    w = [games.default_waves_per_state(A) for A in range(1, 4100)]
    assert min(w) >= 1 and max(w) <= 64
    assert [games.default_waves_per_state(A) for A in (9, 21, 81, 162, 428, 3402)] == [2, 3, 8, 8, 4, 2]


def test_the_unit_is_built_with_the_flags_of_the_playout_unit():
    import importlib.util
    spec = importlib.util.spec_from_file_location('azg_build_surface', os.path.join(ROOT, 'alpha-zero-general_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    units = dict(b.UNITS)
    assert 'azg_lookahead.hip' in units and units['azg_lookahead.hip'] == units['azg_playout.hip']
