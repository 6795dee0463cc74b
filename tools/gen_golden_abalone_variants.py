"""Golden vectors for Abalone's other starting layouts and for dynamic komi, from the REFERENCE (imported live, pure-Python mode) with
its two module constants patched in the temp copy (tools/refshim/harness.load_reference: INITIAL_LAYOUT, ENABLE_DYNAMIC_KOMI of
abalone/AbaloneLogicNumba.py:5-6): the env / symmetry / MCTS families of tools/gen_golden_abalone.py for
    abalone_classic, abalone_german                 (no komi: a score tie at the round limit is the 0.001 draw)
    abalone_classic_komi, abalone_belgian_komi      (misc[0, 3] decides the tie and flips with the seats)
The komi bit of an init board comes from NumPy's generator here and from the engine's counter stream there, so it is no part of the
contract: the tests take the marble planes of init_boards and check the bit against the engine's own rule.  The MCTS roots of the komi
configurations include positions one and two plies before the round limit with level scores, so that terminals decided by the bit,
and children whose canonical form carries the flipped bit, are inside the recorded trees.  The files are written with a fixed member
date (harness.savez): a second run writes the same bytes.  Build-container only:
    python tools/gen_golden_abalone_variants.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'refshim'))
import gen_golden as G  # noqa: E402
import harness as H  # noqa: E402

# name -> (INITIAL_LAYOUT, ENABLE_DYNAMIC_KOMI, offset of the random-play seed: the first for which the file meets check_env -- of eight
# games three to six reach the round limit with level scores, and the bit must have fallen both ways among them)
CONFIGS = {'abalone_classic': (0, False, 0), 'abalone_german': (2, False, 0), 'abalone_classic_komi': (0, True, 0),
           'abalone_belgian_komi': (1, True, 1)}
N_GAMES = 8
for _name, (_layout, _komi, _) in CONFIGS.items():
    G.VARIANTS[_name] = (dict(abalone_layout=_layout, abalone_dynamic_komi=_komi), 'AbaloneGame', 'AbaloneGame')
    G.MCTS_ARGS[_name] = dict(cpuct=1.0, fpu=0.0, universes=0, forced_playouts=True)


def tied_limit_ends(env):
    """rows of the env file where the game ended at the round limit with level scores, and their results"""
    tie = (env['round'] >= 127) & (env['score'][:, 0] == env['score'][:, 1]) & (env['score'].max(axis=1) < 6)
    return env['ended'][tie]


def check_env(name, env):
    """the conditions every file must meet (tests/test_abalone_variants.py checks them again on the committed files)"""
    komi = CONFIGS[name][1]
    ends = tied_limit_ends(env)
    draws = np.isclose(env['ended'], 0.001).any()
    bits = env['state'].reshape(len(env['state']), 81, 4)[:, 3, 3]
    if komi:
        assert not draws, name
        assert (ends == np.float32([1, -1])).all(axis=1).any() and (ends == np.float32([-1, 1])).all(axis=1).any(), (name, ends)
        assert set(np.unique(bits)) == {0, 1}, name
        assert (env['canonical'].reshape(-1, 81, 4)[:, 3, 3] != env['next_state'].reshape(-1, 81, 4)[:, 3, 3]).any(), name
    else:
        assert len(ends) and np.isclose(ends, 0.001).all(), (name, ends)
        assert not bits.any(), name


def late_roots(env, rounds):
    """one not-ended canonical position with level scores per round asked for (the first of the file)"""
    c = env['canonical'].reshape(-1, 81, 4)
    out = []
    for r in rounds:
        sel = np.flatnonzero((c[:, 2, 3] == r) & (c[:, 0, 3] == c[:, 1, 3]) & ~env['ended'].any(axis=1))
        assert len(sel), r
        out.append(env['canonical'][sel[0]].copy())
    return out


def gen_cases(name, roots, n_late, m, game, sims_list):
    """gen_golden.gen_mcts's cases on the roots given (Numba operand typing); the last n_late roots are the late ones"""
    M = m['MCTS']
    H.enable_numba_typing(M)
    P, A, shape = game.num_players, game.getActionSize(), tuple(game.getBoardSize())
    variants = [dict(), dict(universes=1), dict(forced_playouts=False, fpu=0.0), dict(fpu=-0.1, universes=0)]
    cases = []
    for ri, root in enumerate(roots):
        late = ri >= len(roots) - n_late
        for sims in sims_list:
            for var in (variants if ri < 2 else variants[:1]):
                kw = dict(G.MCTS_ARGS[name])
                kw.update(var)
                mc = M.MCTS(game, H.HashNet(P), H.mcts_args(m['utils'], numMCTSSims=sims, **kw))
                board = root.reshape(shape)
                probs, q, full = mc.getActionProb(board, temp=1, force_full_search=True)
                nd = mc.nodes_data[board.tobytes()]
                tied = 0
                for key, node in mc.nodes_data.items():
                    misc = np.frombuffer(key, dtype=np.int8).reshape(81, 4)[:, 3]
                    tied += int(np.asarray(node[0]).any() and misc[0] == misc[1])
                if late:
                    assert tied > 0, (name, ri, sims)
                cases.append(dict(root=root, sims=sims, cpuct=kw['cpuct'], fpu=kw['fpu'], universes=kw['universes'],
                                  forced=int(kw['forced_playouts']), Ns=nd[3], Qs=np.float32(nd[7]),
                                  Nsa=np.asarray(nd[5], dtype=np.int64), Qsa=np.asarray(nd[4], dtype=np.float64),
                                  Ps=np.asarray(nd[2], dtype=np.float32), probs=np.asarray(probs, dtype=np.float64),
                                  q=np.asarray(q, dtype=np.float32), nodes=len(mc.nodes_data), digest=G.tree_digest(mc, A),
                                  tied_terminals=tied, round=int(root.reshape(81, 4)[2, 3])))
    out = {'case_' + k: np.array([c[k] for c in cases]) for k in cases[0]}
    out['typed'] = np.array(1)
    return out


def main():
    for name, (layout, komi, seed) in CONFIGS.items():
        rng = np.random.default_rng(sum(map(ord, name)) + seed)
        env, m, game = G.gen_env(name, N_GAMES, rng, max_plies=140)
        check_env(name, env)
        H.savez(os.path.join(G.GOLDEN, 'env_%s.npz' % name), **env)
        print(name, 'env transitions', len(env['state']), 'tied ends at the limit', tied_limit_ends(env).tolist())
        H.savez(os.path.join(G.GOLDEN, 'sym_%s.npz' % name), **G.gen_sym(name, env, game, rng, 3))
        mid = [env['canonical'][i].copy() for i in rng.choice(len(env['canonical']), size=2, replace=False) if not env['ended'][i].any()]
        late = late_roots(env, (125, 126)) if komi else []
        mc = gen_cases(name, [env['init_boards'][0].copy()] + mid + late, len(late), m, game, [25, 200])
        H.savez(os.path.join(G.GOLDEN, 'mcts_%s_numba.npz' % name), **mc)
        print(name, 'mcts cases', len(mc['case_sims']), 'rounds', sorted(set(mc['case_round'].tolist())), 'tied terminals',
              mc['case_tied_terminals'].tolist())
        H.cleanup()


if __name__ == '__main__':
    main()
