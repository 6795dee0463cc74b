"""CPU: the NumPy restatement of the greedy players (tests/greedyref.py) against the LIVE reference's <G>Players.GreedyPlayer, where the
reference tree is present (skipped elsewhere, like the live half of tests/test_env_coverage.py).  `random.choice` inside the Players
module is replaced by a recorder, GreedyPlayer(game).play runs on the canonicalised envcover rows of greedyref.positions, and the list it
hands to random.choice is the restated candidate set, element for element and in order; for Azul the returned move is the restated one.
This pins the restatement -- and with it azg_greedy_candidates, which tests/test_gpu_greedy.py holds to the restatement -- to the
reference, quirks included (seat 1 of the un-swapped successor, Azul's `if not best_move`).
The branches the rows reach are counted and asserted here, on the CPU, so that the GPU test can rely on them."""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import pytest

import envcover as E
import greedyref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get('AZG_REFERENCE', '/root/reference')
PLAYERS = {'splendor2': 'splendor.SplendorPlayers', 'splendor3': 'splendor.SplendorPlayers', 'abalone': 'abalone.AbalonePlayers',
           'azul': 'azul.AzulPlayers'}


def family(variant):
    return E.VARIANTS[variant][0]


@pytest.mark.parametrize('variant', ['splendor2', 'splendor3'])
def test_splendor_rows_reach_the_branches(variant):
    """the last fallback (no visible card affordable and no gem move valid: every valid id) is counted too; these rows never reach it --
    a position where only reserving or buying a reserved card is possible did not come up in the steered games"""
    og = E.oracle_game(variant)
    count = {'max': 0, 'buy': 0, 'gem': 0, 'all': 0, 'none': 0}
    for b in R.positions(variant):
        valid, scores = R.oracle_scores(og, b)
        count[R.splendor(valid, scores, og.getScore(b.reshape(og.shape), 0))[1]] += 1
    print(variant, count)
    assert count['max'] > 0 and count['buy'] > 0 and count['gem'] > 0 and count['none'] == 0, count
    assert count['all'] == 0, count                                      # (if this ever changes, the docstrings that say so must too)


def test_abalone_rows_have_pushes_and_ties():
    og = E.oracle_game('abalone')
    pushes = ties = 0
    for b in R.positions('abalone'):
        valid, scores = R.oracle_scores(og, b)
        d = scores[valid, 1] - scores[valid, 0]
        pushes += int(d.max() != d.min())
        ties += int(d.max() == d.min())
    print('abalone: positions where a move changes a score', pushes, 'where every d_a ties', ties)
    assert pushes > 0 and ties > 0


def test_azul_rows_have_move_zero_valid():
    og = E.oracle_game('azul')
    zero = kept = 0
    for b in R.positions('azul'):
        valid = og.getValidMoves(b.reshape(og.shape), 0)
        zero += int(valid[0])
        kept += int(valid[0] and R.azul(b, valid) == 0)
    print('azul: positions with move 0 valid', zero, 'where it is the move', kept)
    assert zero >= 8


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason='the reference tree is not on this machine')
@pytest.mark.parametrize('variant', list(PLAYERS))
def test_restatement_equals_the_live_greedy_player(variant):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_golden_envcover as T
    og = E.oracle_game(variant)
    boards = R.positions(variant)
    added = 'colorama' not in sys.modules and importlib.util.find_spec('colorama') is None
    try:
        game = T.ref_game(variant)
        if added:                                                         # (abalone/AbalonePlayers.py colours its HumanPlayer's board with it)
            stub = types.ModuleType('colorama')
            stub.Style = stub.Fore = stub.Back = types.SimpleNamespace()
            sys.modules['colorama'] = stub
        players = importlib.import_module(PLAYERS[variant])
        seen = []

        def choice(seq):
            seen.append(list(seq))
            return seq[0]
        players.random = types.SimpleNamespace(choice=choice)
        player = players.GreedyPlayer(game)
        for i, b in enumerate(boards):
            del seen[:]
            with T.H.CounterRandom(seed=5, stream=i):                     # (Splendor's getNextState(random_seed=0) draws the refill card)
                move = player.play(b.reshape(tuple(game.getBoardSize())).copy(), 0)
            exp = R.candidates('reference', family(variant), og, b, seed=5, stream=i)
            if family(variant) == 'AZUL':
                assert seen == [] and [move] == exp.tolist(), (variant, i, move, exp.tolist())
            else:
                assert len(seen) == 1 and [int(m) for m in seen[0]] == exp.tolist(), (variant, i, seen, exp.tolist())
                assert int(move) == exp[0]
    finally:
        if added:
            sys.modules.pop('colorama', None)
        T.H.cleanup()
