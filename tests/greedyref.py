"""The greedy players' rules restated in NumPy (CPU only), for tests/test_greedy_reference.py -- which holds them to the live reference's
<G>Players.GreedyPlayer on canonicalised envcover rows -- and tests/test_gpu_greedy.py, which holds azg_greedy_candidates and
arena.GreedyContestant to them.  Scores come from the C oracle (or from whoever calls): scores[a] = getScore of every seat on
getNextState(board, 0, a), seats NOT renumbered -- Game.getNextState returns (player + 1) % P without a swap.

reference rules, quirks and all (splendor/SplendorPlayers.py:68-90, abalone/AbalonePlayers.py:182-206, azul/AzulPlayers.py:36-70):
    Splendor  s_a = scores[a][1] (the reference reads seat 1 of the un-swapped board: the opponent), M = max s_a, init = getScore(board, 0):
              M != init -> the valid a with s_a == M ('max'); else the valid ids in [0, 12) ('buy'); else in [30, 60) ('gem'); else all ('all')
    Abalone   the valid a of maximal scores[a][1] - scores[a][0]
    Azul      the reference's loop, literally (`if not best_move` replaces a kept move 0)
lead rule (this project's own, any game): the valid a of maximal scores[a][0] - max_{p >= 1} scores[a][p]."""
import numpy as np

INT32_MIN = -2 ** 31
REFERENCE_GAMES = ('SPLENDOR', 'AZUL', 'ABALONE')


def oracle_scores(og, board, player=0, seed=0, stream=0, counter=0):
    """-> (valid bool[A], scores int64[A, P]: getScore of every seat after each valid move, INT32_MIN in the rows of invalid moves).  Every
    move is stepped with random_seed 0 on a fresh copy of the counter stream (seed, stream) at `counter`: a peek, like azg_env_lookahead."""
    board = np.asarray(board, dtype=np.int8).reshape(og.shape)
    valid = og.getValidMoves(board, player)
    scores = np.full((og.A, og.P), INT32_MIN, dtype=np.int64)
    for a in np.flatnonzero(valid):
        rng = og.rng(seed=seed, stream=stream)
        rng.counter = counter
        nb, _ = og.getNextState(board, player, int(a), 0, rng)
        scores[a] = [og.getScore(nb, p) for p in range(og.P)]
    return valid, scores


def splendor(valid, scores, init):
    """-> (candidate ids in index order, branch: 'max' | 'buy' | 'gem' | 'all' | 'none')"""
    ids = np.flatnonzero(valid)
    if not len(ids):
        return ids, 'none'
    s = scores[ids, 1]
    M = s.max()
    if M != init:
        return ids[s == M], 'max'
    buy = ids[ids < 12]
    if len(buy):
        return buy, 'buy'
    gem = ids[(ids >= 12 + 15 + 3) & (ids < 12 + 15 + 3 + 30)]
    if len(gem):
        return gem, 'gem'
    return ids, 'all'


def abalone(valid, scores):
    ids = np.flatnonzero(valid)
    if not len(ids):
        return ids
    d = scores[ids, 1] - scores[ids, 0]
    return ids[d == d.max()]


def lead(valid, scores):
    ids = np.flatnonzero(valid)
    if not len(ids):
        return ids
    key = scores[ids, 0] - scores[ids, 1:].max(axis=1)
    return ids[key == key.max()]


def azul(board, valid):
    """the loop of azul/AzulPlayers.py:41-70 on the canonical board int8[23, 6] -> the move, or None without a valid one"""
    board = np.asarray(board).reshape(23, 6).astype(np.int64)
    best_move, best_to_line, best_to_floor = None, 0, 0
    for move in range(len(valid)):
        if valid[move]:
            factory = board[3 + (move // 30)]
            colour = (move % 30) // 6
            line = move % 6
            num_tiles = factory[colour]
            if line == 5:
                to_line = 0
                to_floor = num_tiles
            else:
                num_on_line = board[11][line]
                to_line = min(line + 1 - num_on_line, num_tiles)
                to_floor = num_tiles - to_line
            if not best_move:
                best_move, best_to_line, best_to_floor = move, to_line, to_floor
            elif to_line > best_to_line:
                best_move, best_to_line, best_to_floor = move, to_line, to_floor
            elif to_line == best_to_line and to_floor < best_to_floor:
                best_move, best_to_line, best_to_floor = move, to_line, to_floor
    return best_move


def candidates(rule, name, og, board, **stream):
    """the candidate ids (int array, index order) of the canonical `board` under `rule` ('reference' | 'lead') for the oracle game `og` of
    the family `name` ('SPLENDOR', ...); stream: oracle_scores' (seed, stream, counter) of the peek"""
    board = np.asarray(board, dtype=np.int8).reshape(og.shape)
    if rule == 'reference' and name == 'AZUL':
        m = azul(board, og.getValidMoves(board, 0))
        return np.array([] if m is None else [m], dtype=np.int64)
    valid, scores = oracle_scores(og, board, 0, **stream)
    return from_scores(rule, name, og, board, valid, scores)


def from_scores(rule, name, og, board, valid, scores):
    """candidates() of a game other than Azul under its reference rule, from oracle_scores' (valid, scores) of the board"""
    board = np.asarray(board, dtype=np.int8).reshape(og.shape)
    valid = np.asarray(valid).astype(bool)
    if rule == 'lead':
        return lead(valid, scores)
    if name == 'SPLENDOR':
        return splendor(valid, scores, og.getScore(board, 0))[0]
    if name == 'ABALONE':
        return abalone(valid, scores)
    raise ValueError('the reference defines no greedy player for this game')


_positions = {}


def positions(variant, count=48):
    """canonical boards int8[n, S] for the greedy tests, the same on every machine: `count` rows evenly spaced over envcover.rows(variant)
    (every one a position with a valid move), canonicalised by the oracle; for Abalone also 16 rows of envcover.rows_six in which the move
    played ejected a marble (so some successor changes a score); for Azul also 8 rows in which move 0 is valid."""
    import envcover as E
    if (variant, count) in _positions:
        return _positions[variant, count]
    og = E.oracle_game(variant)
    r = E.rows(variant)
    sel = np.unique(np.linspace(0, len(r['action']) - 1, count).astype(np.int64))
    states, players = [r['state'][sel]], [r['player'][sel]]
    if variant == 'abalone':
        r6 = E.rows_six(variant)
        ej = np.flatnonzero(r6['eject'])
        ej = ej[np.unique(np.linspace(0, len(ej) - 1, 16).astype(np.int64))]
        states.append(r6['state'][ej]); players.append(r6['player'][ej])
    if variant == 'azul':
        zero = np.flatnonzero(E.unpack(r['valid'], r['A'])[:, 0])
        zero = np.setdiff1d(zero, sel)
        zero = zero[np.unique(np.linspace(0, len(zero) - 1, 8).astype(np.int64))]
        states.append(r['state'][zero]); players.append(r['player'][zero])
    states, players = np.concatenate(states), np.concatenate(players)
    out = np.stack([og.getCanonicalForm(s.reshape(og.shape), int(p)).reshape(-1) for s, p in zip(states, players)]).astype(np.int8)
    _positions[variant, count] = out
    return out


def mask(ids, A):
    out = np.zeros(A, dtype=np.uint8)
    out[ids] = 1
    return out
