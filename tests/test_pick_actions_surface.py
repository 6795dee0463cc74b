"""CPU-only: the surface of the arena baselines -- azg_pick_actions declared in include/azg.h, exported by the built library and bound by
_lib.py; RandomContestant, PolicyContestant, pick_actions and vs_random importable from azg_amd.arena; the test aid that exposes the
RNG contract's draws declared in include/azg_testaids.h and exported."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'alpha-zero-general_amd', 'libazg_hip.so')


def test_pick_actions_is_declared_exported_and_bound():
    from azg_amd import _lib
    h = open(os.path.join(ROOT, 'include', 'azg.h')).read()
    m = re.search(r'\bint\s+azg_pick_actions\s*\(([^;]*)\)\s*;', h)
    assert m, 'include/azg.h does not declare azg_pick_actions'
    assert len(m.group(1).split(',')) == 11                       # mode, probs, valid, T, A, active, rng_seed, stream0, counters, actions_out, stream
    assert 'azg_pick_actions' in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(LIB), 'azg_pick_actions')
    assert len(_lib.lib().azg_pick_actions.argtypes) == 11
    assert re.search(r'\bint\s+azg_debug_rng_u01\s*\(', open(os.path.join(ROOT, 'include', 'azg_testaids.h')).read())
    assert hasattr(ctypes.CDLL(LIB), 'azg_debug_rng_u01')


def test_arena_exports_the_baseline_contestants():
    from azg_amd import arena
    from azg_amd.arena import BatchedArena, PolicyContestant, RandomContestant, pick_actions, vs_random  # noqa: F401
    assert (arena.PICK_UNIFORM, arena.PICK_ARGMAX, arena.PICK_SAMPLE) == (0, 1, 2)
    assert RandomContestant().mode == arena.PICK_UNIFORM

    class Net:
        def predict_batch(self, boards, valids):
            raise NotImplementedError

    assert PolicyContestant(Net()).mode == arena.PICK_ARGMAX and PolicyContestant(Net(), sample=True).mode == arena.PICK_SAMPLE
    try:
        PolicyContestant(object())
    except TypeError:
        pass
    else:
        raise AssertionError('a net without predict_batch must be refused')
