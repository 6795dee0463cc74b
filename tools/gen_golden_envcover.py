"""The reference's own answers on the rows of tests/envcover.py (whole oracle games steered towards every reachable action id) ->
tests/golden/envcover_<variant>.npz, so that a reference-derived truth for those rows travels with the repository.  Build-container only
(imports the reference live, pure-Python mode, through tools/refshim):
    python tools/gen_golden_envcover.py [variant ...]

Each file holds the rows of selection groups 1-3 (envcover.select: the cover of every id taken, the rows that add a valid id, the last
transition of every game) in selection order, with the fields of env_*.npz -- state, player, valid (packed), action, seed, next_state,
next_player, ended, score, round, canonical -- where everything but state / player / action / seed is what the REFERENCE returned, plus
`row` (the index in envcover.rows), `group` and `dropped`: a file may not exceed MAX_BYTES, so the rows that do not fit are left off the
end and counted there.  tests/test_env_coverage.py imports ref_game / ref_outputs from here for its live comparison.

The games that always draw (envcover.DRAWING: Botanik, Minivilles, The Little Prince): row j steps under
CounterRandom(seed=COVER_SEED, stream=j, counter=counter[j]), the stream row j has in a launch of the env kernels; the files also hold
`counter`, `n_uniforms` and `counter_after`, and the generator asserts that the reference consumed as many uniforms as the oracle.
`<abalone set-up>_six` names the rows of envcover.rows_six / select_six (games won by six marbles) -> envcover_<set-up>_six.npz."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(HERE, 'refshim'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import gen_golden as G  # noqa: E402
import gen_golden_abalone  # noqa: E402,F401   (these four register their variants in G.VARIANTS)
import gen_golden_abalone_variants  # noqa: E402,F401
import gen_golden_akropolis  # noqa: E402,F401
import gen_golden_smallworld  # noqa: E402,F401
import harness as H  # noqa: E402
import envcover as E  # noqa: E402

for _n in (3, 4):                                            # as the main() of the two scripts registers them
    G.VARIANTS['akropolis%d' % _n] = (dict(akropolis_players=_n), 'AkropolisGame', 'AkropolisGame')
    G.VARIANTS['smallworld%d' % _n] = (dict(smallworld_players=_n), 'SmallworldGame', 'SmallworldGame')

G.VARIANTS['botanik'] = (dict(), 'BotanikGame', 'BotanikGame')
for _n in (2, 3, 4):
    G.VARIANTS['minivilles%d' % _n] = (dict(minivilles_players=_n), 'MinivillesGame', 'MinivillesGame')
for _n in (3, 4, 5):
    G.VARIANTS['tlp%d' % _n] = (dict(tlp_players=_n), 'TLPGame', 'TLPGame')

MAX_BYTES = 1000000
REF_FIELDS = ('valid', 'next_state', 'next_player', 'ended', 'score', 'round', 'canonical')


def ref_game(variant):
    """the reference's Game object of the variant, made as the generator of its env_*.npz makes it (the constructors of Akropolis and
    Smallworld draw an init board through np.random.choice / randint: fed constants)"""
    kw, modkey, cls = G.VARIANTS[variant]
    m = H.load_reference(**kw)
    if modkey in ('AkropolisGame', 'SmallworldGame'):
        with H.CounterRandom(injected=[0.5] * 64):
            return getattr(m[modkey], cls)()
    if modkey in ('BotanikGame', 'MinivillesGame', 'TLPGame'):     # (their constructors draw an init board from the global RNG too)
        with H.CounterRandom(seed=777, stream=0):
            return getattr(m[modkey], cls)()
    return getattr(m[modkey], cls)()


def ref_outputs(game, sel):
    """the reference on every row of sel (envcover.take): getValidMoves(state, player), getNextState(state, player, action, seed) and, of
    that next state, getGameEnded / getScore of every player / getRound / getCanonicalForm -> dict of arrays typed like envcover's.
    No step may touch the global RNG: the seeds are the reference's own seeded draws."""
    shape, P = tuple(game.getBoardSize()), game.num_players
    out = {k: [] for k in REF_FIELDS}
    for i in range(len(sel['action'])):
        board, player = sel['state'][i].reshape(shape).copy(), int(sel['player'][i])
        with H.CounterRandom(injected=[]) as cr:
            valid = np.asarray(game.getValidMoves(board.copy(), player)).copy()
            nb, npl = game.getNextState(board.copy(), player, int(sel['action'][i]), random_seed=int(sel['seed'][i]))
            nb = np.asarray(nb).copy()
            out['valid'].append(np.packbits(valid.astype(np.uint8)))
            out['next_state'].append(nb.reshape(-1))
            out['next_player'].append(int(npl))
            out['ended'].append(np.asarray(game.getGameEnded(nb.copy(), npl), dtype=np.float32).copy())
            out['score'].append([int(game.getScore(nb.copy(), p)) for p in range(P)])
            out['round'].append(int(game.getRound(nb.copy())))
            out['canonical'].append(np.asarray(game.getCanonicalForm(nb.copy(), npl)).reshape(-1).copy())
        assert cr.counter == 0, ('the reference drew from the global RNG', i)
    return {k: np.array(v, dtype=E.DTYPES[k]).reshape((len(v),) + np.shape(v[0]) if len(v) else (0,)) for k, v in out.items()}


def ref_outputs_drawing(game, sel):
    """ref_outputs for the rows of envcover.take_drawing: the step of row j draws from the global RNG, replaced by the counter stream
    (COVER_SEED, j) at counter[j]; nothing else may draw.  Also n_uniforms and counter_after, which must be the oracle's."""
    shape, P = tuple(game.getBoardSize()), game.num_players
    out = {k: [] for k in REF_FIELDS + ('n_uniforms', 'counter_after')}
    for j in range(len(sel['action'])):
        board, player, c0 = sel['state'][j].reshape(shape).copy(), int(sel['player'][j]), int(sel['counter'][j])
        with H.CounterRandom(injected=[]) as cr:
            out['valid'].append(np.packbits(np.asarray(game.getValidMoves(board.copy(), player)).astype(np.uint8)))
        assert cr.counter == 0, ('getValidMoves drew from the global RNG', j)
        with H.CounterRandom(seed=E.COVER_SEED, stream=j, counter=c0) as cr:
            nb, npl = game.getNextState(board.copy(), player, int(sel['action'][j]), random_seed=int(sel['seed'][j]))
            nb = np.asarray(nb).copy()
        assert cr.counter - c0 == int(sel['n_uniforms'][j]), ('uniforms consumed: reference, oracle', j, cr.counter - c0, int(sel['n_uniforms'][j]))
        out['n_uniforms'].append(cr.counter - c0); out['counter_after'].append(cr.counter)
        with H.CounterRandom(injected=[]) as cr:
            out['next_state'].append(nb.reshape(-1))
            out['next_player'].append(int(npl))
            out['ended'].append(np.asarray(game.getGameEnded(nb.copy(), npl), dtype=np.float32).copy())
            out['score'].append([int(game.getScore(nb.copy(), p)) for p in range(P)])
            out['round'].append(int(game.getRound(nb.copy())))
            out['canonical'].append(np.asarray(game.getCanonicalForm(nb.copy(), npl)).reshape(-1).copy())
        assert cr.counter == 0, ('the reference drew outside the step', j)
    return {k: np.array(v, dtype=E.DTYPES[k]).reshape((len(v),) + np.shape(v[0]) if len(v) else (0,)) for k, v in out.items()}


def selection(name):
    """(variant, rows, idx, group) of a file name: `<variant>` -> groups 1-3 of select(rows()), `<abalone set-up>_six` -> select_six"""
    if name.endswith('_six'):
        r = E.rows_six(name[:-4])
        idx, group = E.select_six(r)
        return name[:-4], r, idx, group
    r = E.rows(name)
    idx, group = E.select(r)
    return name, r, idx[group <= 3], group[group <= 3]


def fixture(name):
    """-> (arrays of the file, rows dropped).  Rows are cut from the end of the selection order until the file fits."""
    import io
    variant, r, idx, group = selection(name)
    sel = E.take(r, idx)
    game = ref_game(variant)
    ref = (ref_outputs_drawing if variant in E.DRAWING else ref_outputs)(game, sel)
    H.cleanup()
    extra = ('counter',) if variant in E.DRAWING else ()

    def build(n):
        d = dict(state=sel['state'][:n], player=sel['player'][:n], action=sel['action'][:n], seed=sel['seed'][:n], row=idx[:n].astype(np.int32),
                 group=group[:n], dropped=np.array(len(idx) - n), shape=np.array(game.getBoardSize()), A=np.array(r['A']), P=np.array(r['P']))
        d.update({k: sel[k][:n] for k in extra})
        d.update({k: v[:n] for k, v in ref.items()})
        return d

    def size(n):
        buf = io.BytesIO()
        np.savez_compressed(buf, **build(n))
        return buf.tell() + 2048                             # (H.savez writes the same deflate stream; slack for the headers)

    lo, hi = 0, len(idx)
    if size(hi) <= MAX_BYTES:
        lo = hi
    while hi - lo > 1:                                       # largest n that fits
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if size(mid) <= MAX_BYTES else (lo, mid)
    return build(lo), len(idx) - lo


def main():
    for variant in (sys.argv[1:] or list(E.VARIANTS) + list(E.DRAWING) + [v + '_six' for v in E.SIX_GAMES]):
        d, dropped = fixture(variant)
        path = os.path.join(G.GOLDEN, 'envcover_%s.npz' % variant)
        H.savez(path, **d)
        assert os.path.getsize(path) <= MAX_BYTES, (variant, os.path.getsize(path))
        print(variant, 'rows', len(d['action']), 'dropped', dropped, 'ids taken', len(np.unique(d['action'])), 'ended',
              int(d['ended'].any(axis=1).sum()), 'bytes', os.path.getsize(path), flush=True)


if __name__ == '__main__':
    main()
