"""GPU: azg_env_lookahead (csrc/lookahead.hip.h) -- all successors of n positions in one launch -- against the loop of existing launches it
replaces.  For one variant of each of the nine games and splendor4: about 48 positions of the steered oracle games of tests/envcover.py
(chosen on the CPU: rows with a single valid move where the game has them, the row with the most valid moves of the run, rows whose move
ended the game, rows of every seat); the yardstick is, for each action id a valid in any row, one next_state_batch with that action on
all rows (rows where a is not valid step their own first valid move and are ignored) on the same stream0 and counters, then
game_ended_batch -- kernels that tests/test_gpu_env_coverage*.py pin to the oracle.  Every output is bit-equal on the valid (t, a) and
holds its fill value elsewhere.  Also: the oracle directly on 16 rows of three games, waves_per_state 1 / 3 / 64, n = 1, `active` with
holes, counters left as they were, no write without successor_states (raw C-ABI, sentinels), error returns."""
import ctypes as C

import numpy as np
import pytest

import envcover as E

pytestmark = pytest.mark.gpu

VARIANTS = ('splendor2', 'splendor4', 'santorini1', 'azul', 'abalone', 'minivilles2', 'tlp3', 'botanik', 'akropolis', 'smallworld3')
# rows with exactly one valid move among the 48 selected ones, counted on the CPU when the test was written.  The steered games of
# Splendor, Abalone and Akropolis have no such row in any of their transitions: a position there always offers several moves.
SINGLE = {'splendor2': 0, 'splendor4': 0, 'santorini1': 2, 'azul': 5, 'abalone': 0, 'minivilles2': 5, 'tlp3': 20, 'botanik': 3, 'akropolis': 0,
          'smallworld3': 4}
N_ROWS = 48
ORACLE_ROWS = {'splendor2': 16, 'abalone': 16, 'minivilles2': 16}
INT32_MIN = -2 ** 31


def make_game(variant):
    if variant in E.DRAWING:
        import test_gpu_env_coverage_drawing as D
        return D.make_game(variant)
    import test_gpu_env
    return test_gpu_env.make_game(variant)


_rows = {}


def select_rows(variant):
    """CPU: -> dict(state int8[n, S], player int32[n], valid bool[n, A], ends bool[n]: the move the steered game took from the row ended
    it; counts: single, most, ending, seats), n = N_ROWS"""
    if variant in _rows:
        return _rows[variant]
    r = E.rows(variant)
    n, A = len(r['action']), r['A']
    nv = E.unpack(r['valid'], A).sum(axis=1)
    ends = r['ended'].any(axis=1)
    single, ending = np.flatnonzero(nv == 1)[:2], np.flatnonzero(ends)
    ending = ending[np.unique(np.linspace(0, len(ending) - 1, 6).astype(np.int64))]
    head = np.unique(np.concatenate([single, [int(nv.argmax())], ending]))
    rest = np.setdiff1d(np.arange(n), head)
    rest = rest[np.unique(np.linspace(0, len(rest) - 1, N_ROWS - len(head)).astype(np.int64))]
    idx = np.sort(np.concatenate([head, rest]))
    valid = E.unpack(r['valid'][idx], A).astype(bool)
    out = dict(state=np.ascontiguousarray(E.states(r, idx) if variant in E.DRAWING else r['state'][idx]), player=r['player'][idx].astype(np.int32),
               valid=valid, ends=ends[idx], action=r['action'][idx], most=int(nv.max()),
               counts=dict(single=int((valid.sum(axis=1) == 1).sum()), most=int((valid.sum(axis=1) == nv.max()).sum()),
                           ending=int(ends[idx].sum()), seats=len(np.unique(r['player'][idx]))))
    _rows[variant] = out
    return out


def fills(g, n, dev):
    import torch
    return dict(valid=torch.zeros((n, g.A), dtype=torch.uint8, device=dev), scores=torch.full((n, g.A, g.P), INT32_MIN, dtype=torch.int32, device=dev),
                ended=torch.zeros((n, g.A, g.P), dtype=torch.float32, device=dev), next_player=torch.full((n, g.A), -1, dtype=torch.int32, device=dev),
                states=torch.zeros((n, g.A, g.S), dtype=torch.int8, device=dev))


def loop_of_launches(g, st, pl, valid, stream0, counters):
    """the yardstick: what the lookahead replaces, one pair of launches per action id -> the dict of fills() filled on the valid (t, a)"""
    import torch
    dev, n = g.device, st.shape[0]
    exp = fills(g, n, dev)
    vt = torch.from_numpy(valid).to(dev)
    exp['valid'] = vt.to(torch.uint8)
    first = torch.from_numpy(valid.argmax(axis=1).astype(np.int32)).to(dev)
    zero = torch.zeros(n, dtype=torch.int64, device=dev)
    for a in np.flatnonzero(valid.any(axis=0)):
        a = int(a)
        m = vt[:, a]
        acts = torch.where(m, torch.full_like(first, a), first)
        c = None if counters is None else counters.clone()
        ns, npl = g.next_state_batch(st, pl, acts, zero, stream0=stream0, counters=c)
        ended, score, _ = g.game_ended_batch(ns, npl)
        exp['states'][:, a] = torch.where(m[:, None], ns, exp['states'][:, a])
        exp['next_player'][:, a] = torch.where(m, npl, exp['next_player'][:, a])
        exp['ended'][:, a] = torch.where(m[:, None], ended, exp['ended'][:, a])
        exp['scores'][:, a] = torch.where(m[:, None], score, exp['scores'][:, a])
    return exp


def same(variant, what, got, exp, rows=None):
    """every field of a Lookahead equal to the dict exp (on `rows` of exp), bit for bit; a failure names variant, field, row and action"""
    import torch
    for k in ('valid', 'scores', 'ended', 'next_player', 'states'):
        x, y = getattr(got, k), exp[k] if rows is None else exp[k][rows]
        if x is None:
            continue
        assert x.dtype == y.dtype and x.shape == y.shape, (variant, what, k, x.dtype, x.shape, y.shape)
        if k == 'ended':
            x, y = x.view(torch.int32), y.view(torch.int32)
        if not torch.equal(x, y):
            bad = (x != y).reshape(x.shape[0], x.shape[1], -1).any(dim=2).nonzero()[0].tolist()
            raise AssertionError('%s %s, %s: first difference at row %d, action %d: got %r, expected %r'
                                 % (variant, what, k, bad[0], bad[1], x[bad[0], bad[1]].tolist(), y[bad[0], bad[1]].tolist()))


@pytest.mark.parametrize('variant', VARIANTS)
def test_lookahead_equals_the_loop_of_launches(variant):
    import torch
    g, og = make_game(variant), E.oracle_game(variant)
    assert (g.S, g.A, g.P) == (og.S, og.A, og.P)
    d = select_rows(variant)
    n, dev = len(d['player']), g.device
    print(variant, 'rows', n, d['counts'], 'most valid moves', d['most'], 'ids valid somewhere', int(d['valid'].any(axis=0).sum()))
    assert n == N_ROWS and d['counts']['single'] == SINGLE[variant] and d['counts']['most'] >= 1 and d['most'] > 1
    assert d['counts']['ending'] >= 6 and d['counts']['seats'] >= 2 and int((d['player'] != 0).sum()) >= 8, d['counts']
    st, pl = torch.from_numpy(d['state']).to(dev), torch.from_numpy(d['player']).to(dev)
    counters = torch.arange(n, dtype=torch.int64, device=dev) * 5 + 3
    before = counters.clone()
    exp = loop_of_launches(g, st, pl, d['valid'], 11, counters)
    assert torch.equal(counters, before)
    # (the rows whose move ended the steered game were stepped with that game's seed; here the draws are the stream's, so only this:)
    assert int((exp['ended'] != 0).any(dim=2).any(dim=1).sum()) >= 1, 'no successor ends the game'
    got = g.lookahead_batch(st, pl, stream0=11, counters=counters, successor_states=True)
    same(variant, 'default waves_per_state', got, exp)
    assert torch.equal(counters, before), 'the lookahead wrote its counters'
    # the result does not depend on how the work is dealt out
    for w in (1, 3, 64):
        same(variant, 'waves_per_state %d' % w, g.lookahead_batch(st, pl, waves_per_state=w, stream0=11, counters=counters, successor_states=True), exp)
    # without successor states the other outputs are the same
    lean = g.lookahead_batch(st, pl, stream0=11, counters=counters)
    assert lean.states is None
    same(variant, 'without successor states', lean, exp)
    # n = 1: row 0 alone is row 0 of the batch (its stream is stream0 + 0 in both)
    same(variant, 'n = 1', g.lookahead_batch(st[:1], pl[:1], stream0=11, counters=counters[:1], successor_states=True), exp, slice(0, 1))
    # active with holes: the rows of an inactive state hold the fill values, valid included
    active = (torch.arange(n, device=dev) % 3 != 1)
    blank = fills(g, n, dev)
    holes = {k: torch.where(active.reshape((n,) + (1,) * (v.dim() - 1)), v, blank[k]) for k, v in exp.items()}
    same(variant, 'active with holes', g.lookahead_batch(st, pl, active=active, stream0=11, counters=counters, successor_states=True), holes)
    same(variant, 'active as u8', g.lookahead_batch(st, pl, active=active.to(torch.uint8), waves_per_state=2, stream0=11, counters=counters), holes)
    assert g.lookahead_batch(st[:0], pl[:0]).valid.shape == (0, g.A)          # n == 0 launches nothing
    # without counters every peek starts at 0: the oracle itself on a few rows (getValidMoves, getNextState on the row's stream, getScore,
    # getGameEnded)
    k = ORACLE_ROWS.get(variant, 0)
    if k:
        got = g.lookahead_batch(st[:k], pl[:k], stream0=5, successor_states=True)
        got = {f: getattr(got, f).cpu().numpy() for f in got._fields}
        steps = 0
        for t in range(k):
            board, p = d['state'][t].reshape(og.shape), int(d['player'][t])
            valid = og.getValidMoves(board, p)
            assert np.array_equal(got['valid'][t].astype(bool), valid), (variant, t)
            for a in np.flatnonzero(valid):
                nb, npl = og.getNextState(board, p, int(a), 0, og.rng(seed=g.rng_seed, stream=5 + t))
                assert np.array_equal(got['states'][t, a], nb.reshape(-1)) and got['next_player'][t, a] == npl, (variant, t, a)
                assert got['scores'][t, a].tolist() == [og.getScore(nb, q) for q in range(og.P)], (variant, t, a)
                assert np.array_equal(got['ended'][t, a], og.getGameEnded(nb, npl)), (variant, t, a)
                steps += 1
            assert (got['next_player'][t][~valid] == -1).all() and (got['scores'][t][~valid] == INT32_MIN).all()
        assert steps > k


def raw_call(g, st, pl, n, w, bufs, game=None):
    import torch
    from azg_amd._lib import lib
    p = [None if b is None else C.c_void_p(b.data_ptr()) for b in bufs]
    return lib().azg_env_lookahead(g.GAME_ID if game is None else game, g.variant, C.c_void_p(st.data_ptr()), C.c_void_p(pl.data_ptr()), None, n, w,
                                   C.c_uint64(g.rng_seed), C.c_uint64(11), None, p[0], p[1], p[2], p[3], p[4],
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_raw_call_writes_valid_rows_only_and_nothing_without_successor_states():
    """the raw C-ABI on buffers full of a sentinel, each between two guard bands of the same allocation: with out_states NULL the guards
    and every row of an invalid action keep the sentinel, the valid rows are those of the run with successor states"""
    import torch
    g = make_game('splendor2')
    d = select_rows('splendor2')
    n, dev, G = 8, g.device, 4096
    st, pl = torch.from_numpy(d['state'][:n]).to(dev), torch.from_numpy(d['player'][:n]).to(dev)
    ref = g.lookahead_batch(st, pl, stream0=11, successor_states=True)
    spec = (('valid', torch.uint8, (n, g.A), 0x5A), ('scores', torch.int32, (n, g.A, g.P), 0x5A5A5A5A), ('ended', torch.float32, (n, g.A, g.P), -7.5),
            ('next_player', torch.int32, (n, g.A), 0x5A5A5A5A))
    whole = {k: torch.full((2 * G + int(np.prod(shape)),), s, dtype=dt, device=dev) for k, dt, shape, s in spec}
    inner = {k: whole[k][G:G + int(np.prod(shape))].view(shape) for k, dt, shape, s in spec}
    assert raw_call(g, st, pl, n, 3, [inner[k] for k, *_ in spec] + [None]) == 0
    torch.cuda.synchronize()
    valid = ref.valid.bool()
    assert torch.equal(inner['valid'], ref.valid)
    for k, dt, shape, s in spec:
        guard = torch.full((G,), s, dtype=dt, device=dev)
        assert torch.equal(whole[k][:G], guard) and torch.equal(whole[k][-G:], guard), k
        if k != 'valid':
            m = valid.reshape(valid.shape + (1,) * (len(shape) - 2)).expand(shape)
            assert torch.equal(inner[k][m], getattr(ref, k)[m]), k
            assert bool((inner[k][~m] == s).all()), k


def test_error_returns_launch_nothing():
    import torch
    from azg_amd._lib import lib
    g = make_game('splendor2')
    d = select_rows('splendor2')
    n, dev = 4, g.device
    st, pl = torch.from_numpy(d['state'][:n]).to(dev), torch.from_numpy(d['player'][:n]).to(dev)
    f = fills(g, n, dev)
    bufs = [f['valid'], f['scores'], f['ended'], f['next_player'], None]
    for what, rc in (('waves_per_state 0', raw_call(g, st, pl, n, 0, bufs)), ('waves_per_state 65', raw_call(g, st, pl, n, 65, bufs)),
                     ('unknown game', raw_call(g, st, pl, n, 1, bufs, game=99)),
                     ('NULL scores', raw_call(g, st, pl, n, 1, [bufs[0], None] + bufs[2:])),
                     ('NULL valid', raw_call(g, st, pl, n, 1, [None] + bufs[1:]))):
        assert rc < 0 and len(lib().azg_last_error()) > 0, what
    assert b'waves_per_state' in (raw_call(g, st, pl, n, 65, bufs), lib().azg_last_error())[1]
    torch.cuda.synchronize()
    fresh = fills(g, n, dev)
    assert all(torch.equal(f[k], fresh[k]) for k in f)
    with pytest.raises(Exception, match='waves_per_state'):
        g.lookahead_batch(st, pl, waves_per_state=0)
