"""GPU: azg_train_gather_forms (csrc/examples.hip.h) -- a training batch computed from the records: batch row b is virtual row ids[b],
the form k = ids[b] - first_row[g] of the lowest record g with row_end[g] > ids[b].  The yardstick is azg_examples_expand on the same
records and streams (tests/test_gpu_examples_expand.py pins that call to the reference's fixtures): virtual row r must hold, byte for
byte, row r of the expanded columns.  Every output is pre-filled with a guard byte and has three spare rows, so a row written outside
its place shows.  Per game: every virtual row in a shuffled order with repeats at B = 1, 63, 64, 65 and the whole list; n = 1; explicit
non-contiguous streams and streams = NULL; a front window (first_row[0] < 0), a clamped end and two iterations on different bases with
wholly cut records between them; two calls give the same bytes."""
import numpy as np
import pytest

from test_gpu_examples_expand import GUARD, expand, make_game, records

pytestmark = pytest.mark.gpu

# fixture -> records taken from it (the golden files hold 6 / 6 / 2 / 3 / 3 records of Splendor / Santorini / Azul / Abalone / Akropolis)
TAGS = {'splendor2': 6, 'santorini1': 6, 'azul': 2, 'abalone': 3, 'minivilles2': 24, 'botanik': 12, 'akropolis': 3, 'smallworld': 12,
        'tlp3': 16, 'tlp5': 12}
# what the fixture must exercise: the set of form counts (None: the draws decide -- more than one count, none above the candidates)
FORM_COUNTS = {'splendor2': {10, 13, 14}, 'santorini1': {8}, 'azul': {120}, 'abalone': {12}, 'minivilles2': {1}, 'botanik': {13, 14},
               'akropolis': {6}, 'smallworld': {3}, 'tlp3': None, 'tlp5': None}
S0 = (1 << 42) + 17


def gather(g, dev, first_row, row_end, streams, ids):
    """one call into guard-filled outputs of len(ids) + 3 rows -> the five outputs as uint8 [len(ids) + 3, bytes per row] arrays"""
    import torch
    from azg_amd._lib import check, lib
    from azg_amd.games import _ptr, _stream
    d = g.device
    B = len(ids)
    outs = [torch.full((B + 3, w), GUARD, dtype=torch.uint8, device=d)
            for w in (g.S, 4 * g.A, 4 * g.P, g.A, 4 * g.P)]
    t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(np.asarray(x).astype(dt))).to(d)      # noqa: E731
    fr, re_, idt = t(first_row, np.int64), t(row_end, np.int64), t(ids, np.int32)
    st = None if streams is None else t(np.asarray(streams, dtype=np.uint64).view(np.int64), np.int64)
    check(lib().azg_train_gather_forms(g.GAME_ID, g.variant, *[_ptr(x) for x in dev], _ptr(fr), _ptr(re_), None if st is None else _ptr(st),
                                       len(first_row), _ptr(idt), B, *[_ptr(o) for o in outs], g.rng_seed, _stream()))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def check_batch(got, want, ids):
    """rows [0, B) are the yardstick's rows `ids`, the three spare rows keep the guard"""
    B = len(ids)
    for k, (a, w) in enumerate(zip(got, want)):
        assert a.shape == (B + 3, w.shape[1]), k
        assert np.array_equal(a[:B], w[np.asarray(ids, dtype=np.int64)]), 'column %d' % k
        assert (a[B:] == GUARD).all(), 'column %d: a spare row was written' % k


def shuffled_with_repeats(total, seed):
    """every virtual row at least once, shuffled, at least 70 entries"""
    r = np.random.default_rng(seed)
    ids = np.concatenate([r.permutation(total), r.integers(0, total, max(7, 70 - total))])
    r.shuffle(ids)
    return ids.astype(np.int64)


def expanded(g, recs, stream0):
    """the yardstick: (counts, the five expanded columns as uint8 [total, bytes per row])"""
    counts, bufs, _ = expand(g, recs, stream0=stream0)
    total = int(counts.sum())
    return counts, [b[:total] for b in bufs]


def some_records(golden_dir, tag, g, at_least=4, at_most=8):
    """at_least .. at_most records: the fixture's, repeated where it holds fewer -- with z and q drawn anew for every record, so that two
    copies of one state still give different rows"""
    recs = records(golden_dir, tag, g, limit=min(TAGS[tag], at_most))
    n = len(recs[0])
    if n < at_least:
        recs = [np.concatenate([x] * -(-at_least // n))[:at_least] for x in recs]
        r = np.random.default_rng(23)
        recs[2], recs[4] = [r.standard_normal(recs[2].shape).astype(np.float32) for _ in range(2)]
    return [np.ascontiguousarray(x) for x in recs]


def device_records(g, recs):
    import torch
    return [torch.from_numpy(x).to(g.device) for x in recs]


@pytest.mark.parametrize('tag', list(TAGS))
def test_virtual_rows_equal_the_expanded_rows(golden_dir, tag):
    g = make_game(tag, rng_seed=1234)
    recs = records(golden_dir, tag, g, limit=TAGS[tag])
    n = len(recs[0])
    dev = device_records(g, recs)
    counts, want = expanded(g, recs, S0)
    if FORM_COUNTS[tag] is not None:
        assert set(counts.tolist()) == FORM_COUNTS[tag]
    else:
        assert 1 <= counts.min() and counts.max() <= 2 * g.P + 1 and len(set(counts.tolist())) > 1
    total = int(counts.sum())
    ends = np.cumsum(counts)
    first = ends - counts
    streams = (S0 + np.arange(n)).astype(np.uint64)
    ids = shuffled_with_repeats(total, 1)
    assert len(ids) >= 70 and set(ids.tolist()) == set(range(total))
    # every virtual row, shuffled, with repeats: the whole list, then B = 1, 63, 64, 65
    whole = gather(g, dev, first, ends, streams, ids)
    check_batch(whole, want, ids)
    for B in (1, 63, 64, 65):
        check_batch(gather(g, dev, first, ends, streams, ids[:B]), want, ids[:B])
    # two calls give identical bytes
    again = gather(g, dev, first, ends, streams, ids)
    assert all(np.array_equal(a, b) for a, b in zip(whole, again))
    # streams = NULL: record j draws from stream j
    counts0, want0 = expanded(g, recs, 0)
    ends0 = np.cumsum(counts0)
    ids0 = shuffled_with_repeats(int(ends0[-1]), 2)
    check_batch(gather(g, dev, ends0 - counts0, ends0, None, ids0), want0, ids0)
    # n = 1
    one = [x[:1] for x in dev]
    ids1 = shuffled_with_repeats(int(counts[0]), 3)
    check_batch(gather(g, one, first[:1], ends[:1], streams[:1], ids1), [w[:counts[0]] for w in want], ids1)


@pytest.mark.parametrize('tag', list(TAGS))
def test_explicit_streams_that_are_not_contiguous(golden_dir, tag):
    """record j draws from its own stream, whatever its place: the yardstick expands every record alone on that stream"""
    g = make_game(tag, rng_seed=1234)
    recs = some_records(golden_dir, tag, g)
    n = len(recs[0])
    streams = np.array([S0 + 1000 - 37 * j if j % 2 else (1 << 63) + 5 * j for j in range(n)], dtype=np.uint64)
    parts = [expanded(g, [x[j:j + 1] for x in recs], int(streams[j])) for j in range(n)]
    counts = np.array([int(p[0][0]) for p in parts])
    want = [np.concatenate([p[1][k] for p in parts]) for k in range(5)]
    ends = np.cumsum(counts)
    ids = shuffled_with_repeats(int(ends[-1]), 4)
    check_batch(gather(g, device_records(g, recs), ends - counts, ends, streams, ids), want, ids)


@pytest.mark.parametrize('tag', list(TAGS))
def test_windows_and_two_iterations_on_different_bases(golden_dir, tag):
    """Iteration A keeps the rows behind a front cut (record 0 wholly cut, the cut falls inside record 1 where it has more than one
    form: first_row[0] < 0) and loses its last row to a clamp from above; iteration B -- the same records on the streams behind A's --
    starts at A's end with its records 0 and 1 wholly cut, so records that own no row lie between the two.  Virtual row r is row r of
    the two expanded iterations, cut the same way and laid end to end."""
    g = make_game(tag, rng_seed=1234)
    recs = some_records(golden_dir, tag, g)
    n = len(recs[0])
    ca, wa = expanded(g, recs, S0)
    cb, wb = expanded(g, recs, S0 + n)
    ea, eb = np.cumsum(ca), np.cumsum(cb)
    shift_a = int(ca[0]) + 1
    end_a = int(ea[-1]) - shift_a - 1                                      # A's live rows: [0, end_a)
    shift_b = int(cb[0] + cb[1])
    assert end_a > 0 and int(eb[-1]) > shift_b
    first_a = ea - ca - shift_a
    row_end_a = np.clip(np.maximum(first_a + ca, 0), None, end_a)         # clamped from below to the base 0, from above to end_a
    first_b = end_a + eb - cb - shift_b
    row_end_b = np.maximum(first_b + cb, end_a)
    first, row_end = np.concatenate([first_a, first_b]), np.concatenate([row_end_a, row_end_b])
    assert first[0] < 0 and (np.diff(row_end) >= 0).all()
    assert row_end_a[0] == 0 and row_end_b[0] == row_end_b[1] == end_a                               # records that own no row
    streams = (S0 + np.arange(2 * n)).astype(np.uint64)
    want = [np.concatenate([a[shift_a:shift_a + end_a], b[shift_b:]]) for a, b in zip(wa, wb)]
    total = end_a + int(eb[-1]) - shift_b
    assert len(want[0]) == total == row_end[-1]
    dev = device_records(g, [np.concatenate([x, x]) for x in recs])
    ids = shuffled_with_repeats(total, 5)
    check_batch(gather(g, dev, first, row_end, streams, ids), want, ids)
    # in order as well: the first and the last row of either iteration
    edge = np.array([0, end_a - 1, end_a, total - 1])
    check_batch(gather(g, dev, first, row_end, streams, edge), want, edge)


def test_an_id_that_no_record_owns_touches_nothing_outside_its_row(golden_dir):
    """r < 0, r >= row_end[n - 1] and a k beyond the record's forms: the rows are undefined, the rows beside them are not"""
    g = make_game('splendor2')
    recs = records(golden_dir, 'splendor2', g, limit=2)
    counts, want = expanded(g, recs, 0)
    assert counts.tolist() == [14, 10]                                     # (total + 1 is then form 11 of a record with 10 of 14 candidates)
    ends = np.cumsum(counts)
    total = int(ends[-1])
    row_end = ends.copy()
    row_end[-1] += 40                                                      # (a row_end beyond the record's forms: k >= its count)
    ids = np.array([3, -1, total + 45, total + 20, -2 ** 31, 2 ** 31 - 1, 0, total - 1, total + 1, total + 3])
    got = gather(g, device_records(g, recs), ends - counts, row_end, None, ids)
    good, bad = [0, 6, 7], [1, 2, 3, 4, 5, 8, 9]
    for a, w in zip(got, want):
        assert np.array_equal(a[good], w[ids[good]]) and (a[len(ids):] == GUARD).all()
        assert (a[bad] == GUARD).all()                                     # (this build leaves such a row alone; the contract says undefined)


def test_nothing_is_launched_for_an_empty_batch(golden_dir):
    g = make_game('splendor2')
    recs = records(golden_dir, 'splendor2', g, limit=2)
    got = gather(g, device_records(g, recs), [0, 10], [10, 20], None, np.zeros(0, np.int64))
    assert all((a == GUARD).all() and len(a) == 3 for a in got)
