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
oracle is pinned to the reference's seeded draws for these only); the game stops at getGameEnded(...).any().

Two further families (tests/test_env_coverage_drawing.py, tests/test_gpu_env_coverage_drawing.py), each described where it is defined:
DRAWING, the games whose step draws whatever random_seed says (rows_drawing, take_drawing: a counter stream per game, selected rows
re-evaluated on the stream of their place in a launch), and rows_six / select_six, Abalone games steered to a win by six marbles."""
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
    name, v = VARIANTS[variant] if variant in VARIANTS else DRAWING[variant]
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
    if variant in DRAWING:
        return rows_drawing(variant, games)
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
    if 'n_uniforms' in r:                                    # the games that always draw: both the drawing and the non-drawing path of an id
        g1 = np.union1d(g1, np.unique(r['action'].astype(np.int64) * 256 + r['n_uniforms'], return_index=True)[1])
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
    if r['variant'] in DRAWING:
        return take_drawing(r, idx)
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


# ---- the games that always draw: Botanik (deck), Minivilles (dice, purple cards), The Little Prince (market refill) ----------------
# Their step consumes uniforms whatever random_seed says (tests/test_env_coverage_drawing.py checks), so game g is played on the
# stream og.rng(seed=INIT_SEED, stream=g): getInitBoard consumes from it and every step continues it.  A launch of the C-ABI gives
# row j the stream stream0 + j, so a row cannot keep its game's stream: take() re-evaluates the selected row j on
# og.rng(seed=COVER_SEED, stream=j) at the counter the row had in its game, and that is what reference, fixture and kernels are held to.
DRAWING = {'botanik': ('BOTANIK', 0), 'minivilles2': ('MINIVILLES', 2), 'minivilles3': ('MINIVILLES', 3), 'minivilles4': ('MINIVILLES', 4),
           'tlp3': ('TLP', 3), 'tlp4': ('TLP', 4), 'tlp5': ('TLP', 5)}
COVER_SEED = 2718
# Botanik does not saturate under the plain rule (ids taken 230 / 285 / 305 after 200 / 1000 / 1600 games), and a game is about 80 rows
# of 2310 bytes: its run is bounded, steered with a one-ply lookahead, and keeps states only for the rows take() is asked for (replayed)
DRAWING_GAMES = {'botanik': 1000}
LOOKAHEAD_CANDIDATES = 3
DTYPES.update(counter=np.int64, n_uniforms=np.int8, counter_after=np.int64, eject=np.bool_)


def _copy_rng(rng):
    return type(rng).from_buffer_copy(rng)


def _botanik_lookahead(og, board, player, idx, taken, rng, pick):
    """one ply ahead, for the plies at which the plain rule has no untaken id to offer: among (at most LOOKAHEAD_CANDIDATES of) the moves
    that can free a card or place one (ids >= 15), uniform among those whose successor has a valid id the run has not taken; else, with
    probability 0.5 each where there is one, a move that fills a register (ids < 15: a card is freed only from a filled register) or one
    that grows a machine (35..426, not the throw-away 427); else None: the plain rule's uniform choice"""
    far = idx[idx >= 15]
    if len(far) > LOOKAHEAD_CANDIDATES:
        far = far[np.sort(np.argsort([pick.random() for _ in far], kind='stable')[:LOOKAHEAD_CANDIDATES])]
    good = []
    for a in far:
        nb, npl = og.getNextState(board, player, int(a), 0, _copy_rng(rng))
        if (og.getValidMoves(nb, npl) & ~taken).any():
            good.append(int(a))
    if good:
        return good[int(pick.random() * len(good))]
    for cand in (idx[idx < 15], idx[(idx >= 35) & (idx < og.A - 1)]):
        if len(cand) and pick.random() < 0.5:
            return int(cand[int(pick.random() * len(cand))])
    return None


def rows_drawing(variant, games=None, lookahead=None):
    """rows() for a variant of DRAWING: the same steering (probability 0.7 for an untaken id, what the old fixture takes first), game g on
    the stream (INIT_SEED, g) from getInitBoard on; per row also `counter` (of that stream before the step) and `n_uniforms` (consumed by
    the step).  `seed` is recorded as in rows() and changes nothing.  lookahead (None: Botanik only) adds _botanik_lookahead at the plies
    where the plain rule would choose among all valid ids.  Botanik rows carry no state / next_state: states() replays them."""
    games = DRAWING_GAMES.get(variant, 400) if games is None else games
    lookahead = variant == 'botanik' if lookahead is None else lookahead
    if (variant, games, lookahead) in _cache:
        return _cache[variant, games, lookahead]
    og = oracle_game(variant)
    keep_states = variant != 'botanik'
    pick = np.random.default_rng(1)
    taken = np.zeros(og.A, dtype=bool)
    wanted = np.zeros(og.A, dtype=bool)
    wanted[np.unique(np.load(os.path.join(GOLDEN, fixture_name(variant)))['action'])] = True
    keys = ('player', 'valid', 'action', 'seed', 'next_player', 'ended', 'game', 'ply', 'counter', 'n_uniforms')
    rec = {k: [] for k in keys + (('state', 'next_state') if keep_states else ())}
    for g in range(games):
        rng = og.rng(seed=INIT_SEED, stream=g)
        board, player = og.getInitBoard(rng), 0
        for ply in range(MAX_PLIES):
            valid = og.getValidMoves(board, player)
            idx = np.flatnonzero(valid)
            if not len(idx):
                break
            fresh = idx[~taken[idx]]
            first = fresh[wanted[fresh]]
            fresh = first if len(first) else (fresh if pick.random() < 0.7 else fresh[:0])
            a = None
            if lookahead and not len(fresh):
                a = _botanik_lookahead(og, board, player, idx, taken, rng, pick)
            if a is None:
                cand = fresh if len(fresh) else idx
                a = int(cand[int(pick.random() * len(cand))])
            taken[a] = True
            seed, counter = MAGIC_SEEDS[(g + ply) % 8], int(rng.counter)
            nb, npl = og.getNextState(board, player, a, seed, rng)
            ended = og.getGameEnded(nb, npl)
            if keep_states:
                rec['state'].append(board.reshape(-1)); rec['next_state'].append(nb.reshape(-1))
            rec['player'].append(player); rec['valid'].append(np.packbits(valid)); rec['action'].append(a); rec['seed'].append(seed)
            rec['next_player'].append(npl); rec['ended'].append(ended); rec['game'].append(g); rec['ply'].append(ply)
            rec['counter'].append(counter); rec['n_uniforms'].append(int(rng.counter) - counter)
            board, player = nb, npl
            if ended.any():
                break
    out = {k: np.array(v, dtype=DTYPES[k]) for k, v in rec.items()}
    out['A'], out['P'], out['variant'] = og.A, og.P, variant
    _cache[variant, games, lookahead] = out
    return out


def states(r, idx):
    """the states of the rows idx of a DRAWING run: stored, or (Botanik) the games of those rows played again from their actions"""
    if 'state' in r:
        return r['state'][idx]
    og = oracle_game(r['variant'])
    out = np.empty((len(idx), og.S), dtype=np.int8)
    where = {int(i): j for j, i in enumerate(idx)}
    start = np.flatnonzero(r['ply'] == 0)
    for g in np.unique(r['game'][idx]):
        lo = int(start[g])
        hi = int(start[g + 1]) if g + 1 < len(start) else len(r['action'])
        rng = og.rng(seed=INIT_SEED, stream=int(g))
        board = og.getInitBoard(rng)
        for i in range(lo, hi):
            assert int(rng.counter) == r['counter'][i], (g, i)
            if i in where:
                out[where[i]] = board.reshape(-1)
            board, _ = og.getNextState(board, int(r['player'][i]), int(r['action'][i]), 0, rng)
    return out


def take_drawing(r, idx):
    """take() for a DRAWING run: the fields of the rows idx as played (state, player, valid, action, seed, counter, game, ply), and the
    oracle's step of row j -- its position in idx -- on the stream (COVER_SEED, j) at that counter: next_state, next_player, ended,
    score, round, canonical, n_uniforms, counter_after"""
    og = oracle_game(r['variant'])
    out = {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in r.items() if k not in ('state', 'next_state')}
    out['state'] = states(r, idx)
    rec = {k: [] for k in ('next_state', 'next_player', 'ended', 'score', 'round', 'canonical', 'n_uniforms', 'counter_after')}
    for j in range(len(idx)):
        rng = og.rng(seed=COVER_SEED, stream=j)
        rng.counter = int(out['counter'][j])
        nb, npl = og.getNextState(out['state'][j].reshape(og.shape), int(out['player'][j]), int(out['action'][j]), int(out['seed'][j]), rng)
        rec['next_state'].append(nb.reshape(-1)); rec['next_player'].append(npl); rec['ended'].append(og.getGameEnded(nb, npl))
        rec['score'].append([og.getScore(nb, q) for q in range(og.P)]); rec['round'].append(og.getRound(nb))
        rec['canonical'].append(og.getCanonicalForm(nb, npl).reshape(-1))
        rec['n_uniforms'].append(int(rng.counter) - int(out['counter'][j])); rec['counter_after'].append(int(rng.counter))
    out.update({k: np.array(v, dtype=DTYPES[k]).reshape((len(idx),) + np.shape(v[0]) if len(v) else (0,)) for k, v in rec.items()})
    return out


def oracle_outputs_drawing(variant, d, seed=None):
    """the oracle on the rows of d (state, player, action, counter; seed: d's, or one value for every row) with row j on the stream
    (COVER_SEED, j): the fields of oracle_outputs plus n_uniforms and counter_after"""
    og = oracle_game(variant)
    n = len(d['action'])
    r = dict(state=d['state'], player=d['player'], action=d['action'], counter=d['counter'], variant=variant,
             seed=d['seed'] if seed is None else np.full(n, seed, dtype=DTYPES['seed']))
    out = take_drawing(r, np.arange(n))
    out['valid'] = np.array([np.packbits(og.getValidMoves(d['state'][i].reshape(og.shape), int(d['player'][i]))) for i in range(n)],
                            dtype=np.uint8).reshape(n, -1)
    return out


# ---- Abalone: games won by six marbles ------------------------------------------------------------------------------------------
# No game of rows() ends by six (127 steered plies push too rarely), so the s0 >= 6 / s1 >= 6 branch of game_ended and the scores 5
# and 6 need a run of their own, which leaves the rows of rows() where they are.
SHOVE = 0.5
SIX_GAMES = {'abalone': 200, 'abalone_german': 200, 'abalone_belgian_komi': 200, 'abalone_classic': 150, 'abalone_classic_komi': 150}


def rows_six(variant, games=None):
    """rows() steered towards pushes.  A valid move that raises the mover's score is an ejecting id: one that no earlier row of this
    run took as an ejection goes first; otherwise, with probability 0.9, the action is uniform among the ejecting ids; otherwise, with
    probability SHOVE where there is one, uniform among the moves that displace an opposing marble (that is what brings marbles to the
    edge: without it the classic layout gave 4 wins by six in 200 games, under the floor of tests/test_env_coverage_drawing.py);
    otherwise the rule of rows().  Seeded like rows(); the fields of rows() plus `eject` (the row's move raised the mover's score)."""
    games = SIX_GAMES[variant] if games is None else games
    if (variant, games, 'six') in _cache:
        return _cache[variant, games, 'six']
    og = oracle_game(variant)
    pick = np.random.default_rng(1)
    taken = np.zeros(og.A, dtype=bool)
    ejected = np.zeros(og.A, dtype=bool)
    wanted = np.zeros(og.A, dtype=bool)
    wanted[np.unique(np.load(os.path.join(GOLDEN, fixture_name(variant)))['action'])] = True
    rec = {k: [] for k in ('state', 'player', 'valid', 'action', 'seed', 'next_state', 'next_player', 'ended', 'game', 'ply', 'eject')}
    for g in range(games):
        board, player = og.getInitBoard(og.rng(seed=INIT_SEED, stream=g)), 0
        for ply in range(MAX_PLIES):
            valid = og.getValidMoves(board, player)
            idx = np.flatnonzero(valid)
            if not len(idx):
                break
            seed, before = MAGIC_SEEDS[(g + ply) % 8], og.getScore(board, player)
            after = [og.getNextState(board, player, int(a), seed)[0] for a in idx]
            push = idx[[og.getScore(b, player) > before for b in after]]
            shove = idx[[(b[..., 1 - player] != board[..., 1 - player]).any() for b in after]]     # an opposing marble moved
            new = push[~ejected[push]]
            if len(new):
                cand = new
            elif len(push) and pick.random() < 0.9:
                cand = push
            elif len(shove) and pick.random() < SHOVE:
                cand = shove
            else:
                fresh = idx[~taken[idx]]
                first = fresh[wanted[fresh]]
                fresh = first if len(first) else (fresh if pick.random() < 0.7 else fresh[:0])
                cand = fresh if len(fresh) else idx
            a = int(cand[int(pick.random() * len(cand))])
            taken[a] = True
            nb, npl = og.getNextState(board, player, a, seed)
            eject = og.getScore(nb, player) > before
            ejected[a] |= eject
            ended = og.getGameEnded(nb, npl)
            rec['state'].append(board.reshape(-1)); rec['player'].append(player); rec['valid'].append(np.packbits(valid))
            rec['action'].append(a); rec['seed'].append(seed); rec['next_state'].append(nb.reshape(-1)); rec['next_player'].append(npl)
            rec['ended'].append(ended); rec['game'].append(g); rec['ply'].append(ply); rec['eject'].append(eject)
            board, player = nb, npl
            if ended.any():
                break
    out = {k: np.array(v, dtype=DTYPES[k]) for k, v in rec.items()}
    out['A'], out['P'], out['variant'] = og.A, og.P, variant
    _cache[variant, games, 'six'] = out
    return out


def scores_after(r):
    """int[n, P]: getScore of every player on the next_state of every row"""
    og = oracle_game(r['variant'])
    return np.array([[og.getScore(b, p) for p in range(og.P)] for b in r['next_state']], dtype=np.int64).reshape(len(r['action']), og.P)


def select_six(r):
    """-> (idx, group) of rows_six, without repeats, in row order inside a group: 1 the first row that takes each ejecting action id,
    2 every row whose next state has a score of 5 or 6 for either player, 3 the last transition of every game"""
    n = len(r['action'])
    ej = np.flatnonzero(r['eject'])
    g1 = np.sort(ej[np.unique(r['action'][ej], return_index=True)[1]])
    g2 = np.setdiff1d(np.flatnonzero((scores_after(r) >= 5).any(axis=1)), g1)
    last = np.flatnonzero(np.append(r['game'][1:] != r['game'][:-1], True)) if n else np.zeros(0, dtype=np.int64)
    g3 = np.setdiff1d(last, np.concatenate([g1, g2]))
    idx = np.concatenate([g1, g2, g3])
    group = np.concatenate([np.full(len(x), k + 1, dtype=np.int8) for k, x in enumerate((g1, g2, g3))])
    return idx, group
