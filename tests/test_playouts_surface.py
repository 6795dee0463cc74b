"""CPU-only: the surface of the random playouts -- azg_env_playouts declared in include/azg.h, exported by the built library and bound by
_lib.py; HipGame.playouts_batch, arena.random_games and nnet.RolloutEvaluator with their signatures; the evaluator is no pipeline net."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'alpha-zero-general_amd', 'libazg_hip.so')


def signature(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_env_playouts_is_declared_exported_and_bound():
    from azg_amd import _lib
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'azg.h')).read(), flags=re.S)
    m = re.search(r'\bint\s+azg_env_playouts\s*\(([^;]*)\)\s*;', h)
    assert m, 'include/azg.h does not declare azg_env_playouts'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    assert [p.split()[-1].lstrip('*') for p in params] == [
        'game', 'variant', 'states_dev', 'players_dev', 'active_dev', 'n', 'k', 'max_plies', 'rng_seed', 'stream0', 'counters_dev',
        'out_ended_dev', 'out_plies_dev', 'out_status_dev', 'out_states_dev', 'out_players_dev', 'out_actions_dev', 'stream'], params
    assert 'azg_env_playouts' in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(LIB), 'azg_env_playouts')
    assert len(_lib.lib().azg_env_playouts.argtypes) == 18


def test_python_surface():
    from azg_amd import arena, games, nnet
    empty = inspect.Parameter.empty
    assert signature(games.HipGame.playouts_batch) == [
        ('self', empty), ('boards', empty), ('players', None), ('k', 1), ('max_plies', 4096), ('active', None), ('stream0', 0), ('counters', None),
        ('final_boards', False), ('trace', False)]
    assert games.Playouts._fields == ('ended', 'plies', 'status', 'boards', 'players', 'actions')
    assert signature(arena.random_games) == [('game', empty), ('num', empty), ('stream0', 0), ('max_plies', 4096)]
    assert signature(nnet.RolloutEvaluator.__init__) == [
        ('self', empty), ('game', empty), ('n_playouts', 8), ('max_plies', 4096), ('stream0', 1 << 40), ('max_batch', 1)]
    assert signature(nnet.RolloutEvaluator.predict_batch) == [('self', empty), ('boards', empty), ('valids', empty)]
    assert signature(nnet.RolloutEvaluator.predict) == [('self', empty), ('board', empty), ('valid_actions', empty)]
    assert callable(nnet.RolloutEvaluator.clone_buffers)


def test_rollout_evaluator_is_no_pipeline_net():
    """the asynchronous tree pipeline runs engine nets only: an evaluator of this class name, even with static buffers of the right shape,
    gets no row (SelfPlayEngine then runs it on the two-kernel rounds and refuses async_pipe=True)"""
    import torch
    from azg_amd import _lib, forest

    class RolloutEvaluator:
        pi = torch.zeros((8, 21))
        v = torch.zeros((8, 2))

    assert all(not net.match(RolloutEvaluator()) for net in forest.PIPELINE_NETS)
    for game, variant, A in ((_lib.MINIVILLES, 2, 21), (_lib.SPLENDOR, 2, 81), (_lib.SANTORINI, 1, 162)):
        assert forest.pipeline_row(game, variant, True, [RolloutEvaluator()], 8, A) is None
    assert not any('Rollout' in r.name or 'Rollout' in r.net.name for r in forest.PIPELINE_ROWS)
