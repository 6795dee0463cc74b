"""Rows for the env-coverage tests (tests/test_env_coverage.py on the CPU, tests/test_gpu_env_coverage.py on the GPU): whole games played on
the C oracle and steered towards action ids not taken yet, so that valid_moves / make_move / game_ended / canonical form are exercised on
(nearly) every action id a game can reach and on hundreds of final positions, not on the few random games of tests/golden/env_*.npz.

CPU only (numpy + azg_oracle); the same call gives the same rows on every machine:
    rows(variant)              every transition of the steered games (400 of them; Akropolis: GAMES), as a dict of arrays
    select(rows, cap=16384)    (row indices, group 1..4 of each) of the rows the tests use, in a fixed order
    take(rows, idx)            the rows `idx` with every field of env_*.npz

The recipe of rows(): game g starts from og.getInitBoard(og.rng(seed=99, stream=g)) with player 0 and lasts at most 400 plies; at each
ply, with probability 0.7 (np.random.default_rng(1)) the action is uniform among the valid ids that no earlier row of this run took, if
there is one, otherwise uniform among all valid ids -- but a valid id that the variant's env_*.npz fixture takes and this run has not
yet taken goes first, so that the run covers what the old fixture covers; random_seed = MAGIC_SEEDS[(g + ply) % 8] (the eight seeds of MCTS.py:14 -- the
oracle is pinned to the reference's seeded draws for these only); the game stops at getGameEnded(...).any()."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MAGIC_SEEDS = (31416, 1, 14142, 42, 27183, 2, 16180, 7)      # = tools/refshim/harness.MAGIC_SEEDS (tests/test_env_coverage.py checks)
MAX_PLIES = 400
INIT_SEED = 99

# variant -> (oracle game name, variant of the game family).  The first 13 are VARIANTS of tests/test_gpu_env.py.
VARIANTS = {'splendor2': ('SPLENDOR', 2), 'splendor3': ('SPLENDOR', 3), 'splendor4': ('SPLENDOR', 4), 'santorini1': ('SANTORINI', 1),
            'santorini11': ('SANTORINI', 11), 'azul': ('AZUL', 0), 'abalone': ('ABALONE', ('belgian', False)),
            'akropolis': ('AKROPOLIS', 2), 'akropolis3': ('AKROPOLIS', 3), 'akropolis4': ('AKROPOLIS', 4),
            'smallworld': ('SMALLWORLD', 2), 'smallworld3': ('SMALLWORLD', 3), 'smallworld4': ('SMALLWORLD', 4),
            # the other Abalone set-ups with env_abalone_*.npz fixtures: (layout, dynamic komi)
            'abalone_classic': ('ABALONE', ('classic', False)), 'abalone_german': ('ABALONE', ('german', False)),
            'abalone_classic_komi': ('ABALONE', ('classic', True)), 'abalone_belgian_komi': ('ABALONE', ('belgian', True))}
# games whose env step draws (tile refills, decks, dice): random_seed == 0 takes the counter stream there
STOCHASTIC = ('splendor', 'azul', 'akropolis', 'smallworld')
DTYPES = dict(state=np.int8, player=np.int8, valid=np.uint8, action=np.int16, seed=np.int32, next_state=np.int8, next_player=np.int8,
              ended=np.float32, score=np.int16, round=np.int16, canonical=np.int8, game=np.int32, ply=np.int32)


def oracle_game(variant):
    import azg_oracle as O
    name, v = VARIANTS[variant]
    if name == 'ABALONE':
        from azg_amd.games import abalone_variant
        v = abalone_variant(*v)[2]
    return O.OracleGame(getattr(O, name), v)


def fixture_name(variant):
    return 'env_%s.npz' % variant


# whole games per run.  Akropolis keeps reaching new ids with more games (a far cell needs a city grown towards it, an expensive slot
# needs saved stones); with four players 800 games is where the run covers every id that env_akropolis4.npz takes.
GAMES = {'akropolis4': 800}
_cache = {}


def rows(variant, games=None):
    """every transition of `games` steered oracle games (None: GAMES, else 400): dict of state int8[n, S], player, valid (np.packbits
    rows), action, seed, next_state, next_player, ended f32[n, P], game, ply.  take() adds score, round and canonical form."""
    games = GAMES.get(variant, 400) if games is None else games
    if (variant, games) in _cache:
        return _cache[variant, games]
    og = oracle_game(variant)
    pick = np.random.default_rng(1)                          # (only .random() is used: the same doubles on every NumPy)
    taken = np.zeros(og.A, dtype=bool)
    wanted = np.zeros(og.A, dtype=bool)                      # what the old fixture takes: must be covered here too
    wanted[np.unique(np.load(os.path.join(GOLDEN, fixture_name(variant)))['action'])] = True
    rec = {k: [] for k in ('state', 'player', 'valid', 'action', 'seed', 'next_state', 'next_player', 'ended', 'game', 'ply')}
    for g in range(games):
        board, player = og.getInitBoard(og.rng(seed=INIT_SEED, stream=g)), 0
        for ply in range(MAX_PLIES):
            valid = og.getValidMoves(board, player)
            idx = np.flatnonzero(valid)
            if not len(idx):
                break
            fresh = idx[~taken[idx]]
            first = fresh[wanted[fresh]]
            fresh = first if len(first) else (fresh if pick.random() < 0.7 else fresh[:0])
            cand = fresh if len(fresh) else idx
            a = int(cand[int(pick.random() * len(cand))])
            taken[a] = True
            seed = MAGIC_SEEDS[(g + ply) % 8]
            nb, npl = og.getNextState(board, player, a, seed)
            ended = og.getGameEnded(nb, npl)
            rec['state'].append(board.reshape(-1)); rec['player'].append(player); rec['valid'].append(np.packbits(valid))
            rec['action'].append(a); rec['seed'].append(seed); rec['next_state'].append(nb.reshape(-1)); rec['next_player'].append(npl)
            rec['ended'].append(ended); rec['game'].append(g); rec['ply'].append(ply)
            board, player = nb, npl
            if ended.any():
                break
    out = {k: np.array(v, dtype=DTYPES[k]) for k, v in rec.items()}
    out['A'], out['P'], out['variant'] = og.A, og.P, variant
    _cache[variant, games] = out
    return out


def unpack(valid, A):
    return np.unpackbits(valid, axis=1)[:, :A]


def first_valid(r):
    """for every action id the first row in which it is valid (-1: in none)"""
    A, n = r['A'], len(r['action'])
    first = np.full(A, -1, dtype=np.int64)
    for lo in range(0, n, 4096):
        m = unpack(r['valid'][lo:lo + 4096], A)
        new = m.any(axis=0) & (first < 0)
        first[new] = lo + m[:, new].argmax(axis=0)
    return first


def select(r, cap=16384, spaced=None):
    """-> (idx, group): the rows the tests use, without repeats, group by group and in row order inside a group:
    1  the first row that takes each action id (a cover of everything taken),
    2  the first row in which an action id is valid that is valid in no row selected before it,
    3  the last transition of every game that ended,
    4  other rows, evenly spaced, until `cap` rows are selected (`spaced`: at most that many of them -- for the slow live reference)."""
    n, A = len(r['action']), r['A']
    _, g1 = np.unique(r['action'], return_index=True)
    g1 = np.sort(g1)
    seen = unpack(r['valid'][g1], A).any(axis=0)
    fv = first_valid(r)
    g2 = np.setdiff1d(np.unique(fv[(fv >= 0) & ~seen]), g1)           # (equal to the row-by-row greedy pass: see DESIGN.md §5)
    g3 = np.setdiff1d(np.flatnonzero(r['ended'].any(axis=1)), np.concatenate([g1, g2]))
    head = np.concatenate([g1, g2, g3])
    rest = np.setdiff1d(np.arange(n), head)
    room = max(0, cap - len(head)) if spaced is None else max(0, min(spaced, cap - len(head)))
    g4 = rest if len(rest) <= room else rest[np.unique(np.linspace(0, len(rest) - 1, room).astype(np.int64))] if room else rest[:0]
    idx = np.concatenate([head, g4])[:cap]
    group = np.concatenate([np.full(len(x), k + 1, dtype=np.int8) for k, x in enumerate((g1, g2, g3, g4))])[:cap]
    return idx, group


def take(r, idx):
    """the rows idx of every field of rows(), plus what the oracle says of their next_state: score int16[n, P], round, canonical"""
    out = {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in r.items()}
    og = oracle_game(r['variant'])
    ns, npl = out['next_state'], out['next_player']
    out['score'] = np.array([[og.getScore(b, p) for p in range(og.P)] for b in ns], dtype=DTYPES['score']).reshape(len(ns), og.P)
    out['round'] = np.array([og.getRound(b) for b in ns], dtype=DTYPES['round'])
    out['canonical'] = np.array([og.getCanonicalForm(b, int(p)) for b, p in zip(ns, npl)], dtype=np.int8).reshape(len(ns), -1)
    return out


def counts(r, idx=None):
    """(distinct ids taken, distinct ids ever valid, rows whose game ended) of the rows idx (None: all)"""
    s = r if idx is None else {k: r[k][idx] for k in ('action', 'valid', 'ended')}
    return (len(np.unique(s['action'])), int(unpack(s['valid'], r['A']).any(axis=0).sum()) if len(s['action']) else 0,
            int(s['ended'].any(axis=1).sum()))


def first_diff(got, exp):
    """(row, byte, got, exp) of the first differing element of two arrays of one shape whose first axis is the row; None if equal"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    ne = np.flatnonzero((got != exp).reshape(len(got), -1).any(axis=1)) if got.ndim > 1 else np.flatnonzero(got != exp)
    if not len(ne):
        return None
    i = int(ne[0])
    if got.ndim == 1:
        return i, 0, got[i].item(), exp[i].item()
    j = int(np.flatnonzero(got[i].reshape(-1) != exp[i].reshape(-1))[0])
    return i, j, got[i].reshape(-1)[j].item(), exp[i].reshape(-1)[j].item()


def check_equal(variant, what, got, exp, actions, rows_idx=None):
    """assert got == exp, naming the variant, the row (and its index in rows()), the action id of that row and the first differing byte"""
    d = first_diff(got, exp)
    if d is not None:
        i, j, a, b = d
        n_bad = int((np.asarray(got) != np.asarray(exp)).reshape(len(got), -1).any(axis=1).sum())
        raise AssertionError('%s %s: row %d%s action %d, first differing byte %d: got %r, expected %r (%d of %d rows differ)'
                             % (variant, what, i, '' if rows_idx is None else ' (row %d of rows())' % int(rows_idx[i]), int(actions[i]),
                                j, a, b, n_bad, len(got)))


def oracle_outputs(variant, d):
    """the oracle on the rows of d (state, player, action, seed): valid (packed), next_state, next_player, ended, score, round, canonical"""
    og = oracle_game(variant)
    out = {k: [] for k in ('valid', 'next_state', 'next_player', 'ended', 'score', 'round', 'canonical')}
    for i in range(len(d['action'])):
        b, p = d['state'][i].reshape(og.shape), int(d['player'][i])
        out['valid'].append(np.packbits(og.getValidMoves(b, p)))
        nb, npl = og.getNextState(b, p, int(d['action'][i]), int(d['seed'][i]))
        out['next_state'].append(nb.reshape(-1)); out['next_player'].append(npl); out['ended'].append(og.getGameEnded(nb, npl))
        out['score'].append([og.getScore(nb, q) for q in range(og.P)]); out['round'].append(og.getRound(nb))
        out['canonical'].append(og.getCanonicalForm(nb, npl).reshape(-1))
    return {k: np.array(v, dtype=DTYPES[k]) for k, v in out.items()}
