"""GPU: azg_examples_expand (csrc/examples.hip.h) -- n drained records -> the dense rows of the five example columns in one launch.
Against the reference's own get_symmetries outputs (tests/golden/sym_*.npz) for the games whose forms are deterministic; against the
existing path (HipGame.symmetries_batch + the compaction of Coach._collect) on the same streams for the games whose forms are built or
drawn; and the edges of the row addressing: n = 0 and 1, an order, a base row, a window shorter than the output at both ends -- every
destination buffer is pre-filled with a guard byte and compared as bytes, so a row written outside its place shows."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 0x5A
# fixture -> (constructor name, constructor arguments)
GOLDEN_GAMES = {'splendor2': ('SplendorGame', dict(num_players=2)), 'splendor3': ('SplendorGame', dict(num_players=3)),
                'splendor4': ('SplendorGame', dict(num_players=4)), 'santorini1': ('SantoriniGame', dict(nb_gods=1)),
                'santorini11': ('SantoriniGame', dict(nb_gods=11)), 'azul': ('AzulGame', {}), 'abalone': ('AbaloneGame', {}),
                'abalone_classic': ('AbaloneGame', dict(layout='classic')), 'abalone_german': ('AbaloneGame', dict(layout='german')),
                'abalone_classic_komi': ('AbaloneGame', dict(layout='classic', dynamic_komi=True)),
                'abalone_belgian_komi': ('AbaloneGame', dict(layout='belgian', dynamic_komi=True)),
                'akropolis': ('AkropolisGame', dict(num_players=2)), 'akropolis3': ('AkropolisGame', dict(num_players=3)),
                'akropolis4': ('AkropolisGame', dict(num_players=4))}
BUILT_GAMES = {'tlp3': ('TLPGame', dict(num_players=3)), 'tlp4': ('TLPGame', dict(num_players=4)), 'tlp5': ('TLPGame', dict(num_players=5)),
               'smallworld': ('SmallworldGame', dict(num_players=2)), 'smallworld3': ('SmallworldGame', dict(num_players=3)),
               'smallworld4': ('SmallworldGame', dict(num_players=4)), 'botanik': ('BotanikGame', {}),
               'minivilles2': ('MinivillesGame', dict(num_players=2)), 'minivilles3': ('MinivillesGame', dict(num_players=3)),
               'minivilles4': ('MinivillesGame', dict(num_players=4))}


def make_game(tag, **kw):
    from azg_amd import games
    name, args = {**GOLDEN_GAMES, **BUILT_GAMES}[tag]
    return getattr(games, name)(**args, **kw)


def records(golden_dir, tag, g, limit=None):
    """(states, pi, z, valids, q) as numpy arrays: the fixture's triples with arbitrary z and q"""
    if tag.startswith('minivilles'):
        d = np.load(os.path.join(golden_dir, 'env_%s.npz' % tag))
        st = d['state'].reshape(len(d['state']), -1)[:24]
        va = np.unpackbits(d['valid'], axis=1)[:24, :g.A].astype(np.uint8)
        pi = (np.random.default_rng(5).random(va.shape, dtype=np.float32) * va).astype(np.float32)
    else:
        d = np.load(os.path.join(golden_dir, 'sym_%s.npz' % tag))
        st, pi = d['state'].reshape(len(d['state']), -1), d['pi']
        va = d['valid' if 'valid' in d.files else 'valids'].astype(np.uint8)
    st, pi, va = st[:limit], pi[:limit], va[:limit]
    r = np.random.default_rng(11)
    n = len(st)
    return [np.ascontiguousarray(st.astype(np.int8)), np.ascontiguousarray(pi.astype(np.float32)), r.standard_normal((n, g.P)).astype(np.float32),
            np.ascontiguousarray(va), r.standard_normal((n, g.P)).astype(np.float32)]


def call(g, dev_recs, n, order, first_row, row_begin, row_end, outs, cnt, stream0):
    from azg_amd._lib import check, lib
    from azg_amd.games import _ptr, _stream
    check(lib().azg_examples_expand(g.GAME_ID, g.variant, *[_ptr(t) for t in dev_recs], n, _ptr(order), _ptr(first_row), row_begin, row_end,
                                    *[_ptr(t) for t in outs], _ptr(cnt), g.rng_seed, stream0, _stream()))


def expand(g, recs, order=None, base=0, shift=0, tail=3, window=None, stream0=0):
    """count pass + prefix sum + write pass into guard-filled buffers of base + total - shift + tail rows; form 0 of group j goes to row
    base + (forms before it) - shift.  window = (row_begin, row_end), default every row of the buffers.
    -> (counts, the five buffers as uint8 [rows, bytes per row] arrays, first rows)"""
    import torch
    dev = g.device
    n = len(recs[0])
    dev_recs = [torch.from_numpy(x).to(dev) for x in recs]
    d_order = None if order is None else torch.as_tensor(np.asarray(order, dtype=np.int32)).to(dev)
    cnt = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
    call(g, dev_recs, n, d_order, None, 0, 0, [None] * 5, cnt, stream0)
    counts = cnt.cpu().numpy()[:n].astype(np.int64)
    first = base - shift + np.concatenate([[0], np.cumsum(counts)[:-1]]) if n else np.zeros(0, np.int64)
    rows = base + int(counts.sum()) - shift + tail
    outs = [torch.full((rows, w), GUARD, dtype=torch.uint8, device=dev).view(dt).reshape(rows, -1)
            for w, dt in ((g.S, torch.int8), (4 * g.A, torch.float32), (4 * g.P, torch.float32), (g.A, torch.uint8), (4 * g.P, torch.float32))]
    cnt2 = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
    lo, hi = window if window is not None else (0, rows)
    call(g, dev_recs, n, d_order, torch.from_numpy(first.astype(np.int64)).to(dev) if n else None, lo, hi, outs, cnt2, stream0)
    torch.cuda.synchronize()
    assert np.array_equal(cnt2.cpu().numpy()[:n], counts), 'the write pass counts what the count pass counted'
    return counts, [o.contiguous().view(torch.uint8).reshape(rows, -1).cpu().numpy() for o in outs], first


def expected_rows(forms, recs, src=None):
    """forms[j] = (states [k, S], pi [k, A], valids [k, A]) of group j -> the five columns as uint8 [total, bytes per row] arrays"""
    src = range(len(forms)) if src is None else src
    cols = [[], [], [], [], []]
    for j, (s, p, v) in zip(src, forms):
        k = len(s)
        for c, x in zip(cols, (s.astype(np.int8), p.astype(np.float32), np.repeat(recs[2][j][None], k, 0), v.astype(np.uint8), np.repeat(recs[4][j][None], k, 0))):
            c.append(np.ascontiguousarray(x).reshape(k, -1).view(np.uint8).reshape(k, -1))
    return [np.concatenate(c) for c in cols]


def check_rows(bufs, want, base=0, shift=0, window=None):
    """rows [base, base + total - shift) hold want[shift:], cut to the window; every other byte is the guard"""
    for b, w in zip(bufs, want):
        exp = np.full_like(b, GUARD)
        exp[base:base + len(w) - shift] = w[shift:]
        if window is not None:
            exp[:window[0]] = GUARD
            exp[window[1]:] = GUARD
        assert np.array_equal(b, exp)


def golden_forms(golden_dir, tag, n=None):
    d = np.load(os.path.join(golden_dir, 'sym_%s.npz' % tag))
    vk = 'out_valid' if 'out_valid' in d.files else 'out_valids'
    m = len(d['count']) if n is None else n
    return [(d['out_state'][i][:int(d['count'][i])].reshape(int(d['count'][i]), -1), d['out_pi'][i][:int(d['count'][i])],
             d[vk][i][:int(d['count'][i])]) for i in range(m)], d['count'][:m].astype(np.int64)


def existing_forms(g, recs, stream0):
    """HipGame.symmetries_batch on the same streams, cut to its counts (what the compaction of Coach._collect keeps)"""
    import torch
    ob, op, ov, cnt = g.symmetries_batch(*[torch.from_numpy(recs[k]).to(g.device) for k in (0, 1, 3)], stream0=stream0)
    ob, op, ov, cnt = ob.cpu().numpy(), op.cpu().numpy(), ov.cpu().numpy(), cnt.cpu().numpy().astype(np.int64)
    return [(ob[i, :cnt[i]], op[i, :cnt[i]], ov[i, :cnt[i]]) for i in range(len(cnt))], cnt


@pytest.mark.parametrize('tag', list(GOLDEN_GAMES))
def test_rows_equal_the_references_own_forms(golden_dir, tag):
    g = make_game(tag)
    recs = records(golden_dir, tag, g)
    forms, want_cnt = golden_forms(golden_dir, tag)
    counts, bufs, _ = expand(g, recs)
    assert np.array_equal(counts, want_cnt)
    check_rows(bufs, expected_rows(forms, recs))
    if tag == 'azul':
        assert (counts == 120).all()                                   # count == K: the last form is a row like any other
    if tag.startswith('splendor'):
        assert len(set(counts.tolist())) > 1                           # counts that differ within one call


@pytest.mark.parametrize('tag', list(BUILT_GAMES))
def test_rows_equal_the_existing_path_on_the_same_streams(golden_dir, tag):
    g = make_game(tag, rng_seed=1234)
    recs = records(golden_dir, tag, g, limit=32)
    s0 = (1 << 42) + 17
    forms, want_cnt = existing_forms(g, recs, s0)
    counts, bufs, _ = expand(g, recs, stream0=s0)
    assert np.array_equal(counts, want_cnt)
    check_rows(bufs, expected_rows(forms, recs))
    if tag.startswith('minivilles'):
        assert (counts == 1).all()
    if tag == 'tlp3':
        assert len(set(counts.tolist())) > 1
        other, _ = existing_forms(g, recs, s0 + 1)                      # (the streams matter: another stream0 gives other forms)
        assert any(len(a[0]) != len(b[0]) or not np.array_equal(a[0], b[0]) for a, b in zip(forms, other))


def test_nothing_is_launched_and_nothing_touched_for_no_record(golden_dir):
    import torch
    g = make_game('splendor2')
    recs = [x[:0] for x in records(golden_dir, 'splendor2', g)]
    counts, bufs, _ = expand(g, recs, base=2)
    assert len(counts) == 0
    check_rows(bufs, [np.zeros((0, b.shape[1]), np.uint8) for b in bufs], base=2)
    # ... with live pointers as well: the count buffer keeps its content
    dev_recs = [torch.zeros((1, w), dtype=dt, device=g.device) for w, dt in ((g.S, torch.int8), (g.A, torch.float32), (g.P, torch.float32),
                                                                               (g.A, torch.uint8), (g.P, torch.float32))]
    outs = [torch.full_like(t, 3) for t in dev_recs]
    cnt = torch.full((1,), -7, dtype=torch.int32, device=g.device)
    call(g, dev_recs, 0, None, torch.zeros(1, dtype=torch.int64, device=g.device), 0, 1, outs, cnt, 0)
    torch.cuda.synchronize()
    assert int(cnt.item()) == -7 and all(bool((o == 3).all()) for o in outs)


@pytest.mark.parametrize('tag', ['splendor2', 'tlp3'])
def test_one_record_a_base_row_and_an_order(golden_dir, tag):
    g = make_game(tag, rng_seed=1234)
    recs = records(golden_dir, tag, g, limit=12)
    s0 = 99
    n = len(recs[0])
    forms, want_cnt = existing_forms(g, recs, s0) if tag == 'tlp3' else golden_forms(golden_dir, tag, n)
    want = expected_rows(forms, recs)
    # n = 1
    counts, bufs, _ = expand(g, [x[:1] for x in recs], stream0=s0)
    assert counts.tolist() == [want_cnt[0]]
    check_rows(bufs, [w[:want_cnt[0]] for w in want])
    # a non-zero base row: the rows in front of first_row[0] and behind the last form keep the guard
    counts, bufs, first = expand(g, recs, base=5, tail=4, stream0=s0)
    assert first[0] == 5 and np.array_equal(counts, want_cnt)
    check_rows(bufs, want, base=5)
    # a reversed order against the same call on inputs permuted beforehand: group j expands record n - 1 - j and draws from stream
    # s0 + j, the GROUP's -- so the reference is the existing path on the permuted inputs
    rev = np.arange(n)[::-1].copy()
    perm = [np.ascontiguousarray(x[rev]) for x in recs]
    counts_o, bufs_o, _ = expand(g, recs, order=rev, stream0=s0)
    counts_p, bufs_p, _ = expand(g, perm, stream0=s0)
    assert np.array_equal(counts_o, counts_p) and all(np.array_equal(a, b) for a, b in zip(bufs_o, bufs_p))
    forms_p, cnt_p = existing_forms(g, perm, s0) if tag == 'tlp3' else ([forms[i] for i in rev], want_cnt[rev])
    assert np.array_equal(counts_o, cnt_p)
    check_rows(bufs_o, expected_rows(forms_p, perm))


@pytest.mark.parametrize('tag', ['splendor2', 'tlp3', 'azul'])
def test_a_window_shorter_than_the_output_at_both_ends(golden_dir, tag):
    """deque(maxlen) in rows: first_row shifted down by the surplus (negative for the first groups: a group is cut in the middle) and
    row_end inside the last group -- exactly the rows inside the window are written, the counts are those of the whole output"""
    g = make_game(tag, rng_seed=1234)
    recs = records(golden_dir, tag, g, limit=8)
    s0 = 7
    n = len(recs[0])
    forms, want_cnt = existing_forms(g, recs, s0) if tag == 'tlp3' else golden_forms(golden_dir, tag, n)
    want = expected_rows(forms, recs)
    total = int(want_cnt.sum())
    shift = int(want_cnt[0]) + 1                                        # group 0 and the first form of group 1 fall in front of the window
    cut = 1                                                             # the last form of the last group falls behind it
    assert want_cnt[1] > 1 and want_cnt[-1] > cut
    base = 1
    window = (base, base + total - shift - cut)
    counts, bufs, first = expand(g, recs, base=base, shift=shift, tail=cut + 2, window=window, stream0=s0)
    assert np.array_equal(counts, want_cnt) and first[0] == base - shift < 0
    check_rows(bufs, want, base=base, shift=shift, window=window)
    # an empty window writes nothing at all
    counts, bufs, _ = expand(g, recs, base=base, window=(4, 4), stream0=s0)
    assert np.array_equal(counts, want_cnt)
    assert all((b == GUARD).all() for b in bufs)


def test_refusals():
    import torch
    from azg_amd._lib import AzgError
    g = make_game('splendor2')
    t = torch.zeros(512, dtype=torch.uint8, device=g.device)
    with pytest.raises(AzgError, match='row_end'):
        call(g, [t] * 5, 1, None, None, 3, 2, [t] * 5, t, 0)
    with pytest.raises(AzgError, match='azg_examples_expand'):
        call(g, [None] * 5, 1, None, None, 0, 0, [t] * 5, t, 0)
    g.variant = 9
    with pytest.raises(AzgError):
        call(g, [t] * 5, 1, None, None, 0, 0, [t] * 5, t, 0)
