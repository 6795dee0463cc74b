"""CPU-only: the surface of the compact example history -- azg_train_gather_forms declared in include/azg.h, exported by the built library
and bound by _lib.py, its refusals before any launch; history.CompactHistory's index arithmetic on CPU tensors (append with and without
maxlen, pop_oldest, truncate_iteration, the record file) against a brute-force list of (record, form) per virtual row; and the error
paths: the host trainer given a compact history, Coach('compact') without device_batches, a bad examples_file, a file of expanded rows
loaded into a compact history, an rng_seed that changes between appends."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_kernel_resources import LIB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, A, P = 6, 5, 2
GAME = SimpleNamespace(GAME_ID=1, variant=2, rng_seed=77)


def test_gather_forms_is_declared_exported_and_bound():
    from azg_amd import _lib
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'azg.h')).read(), flags=re.S)
    m = re.search(r'\bint\s+azg_train_gather_forms\s*\(([^;]*)\)\s*;', h)
    assert m, 'include/azg.h does not declare azg_train_gather_forms'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    assert [p.split()[-1].lstrip('*') for p in params] == [
        'game', 'variant', 'states_dev', 'pi_dev', 'z_dev', 'valids_dev', 'q_dev', 'first_row_dev', 'row_end_dev', 'streams_dev', 'n', 'ids_dev',
        'B', 'out_boards_dev', 'out_pi_dev', 'out_z_dev', 'out_valids_dev', 'out_q_dev', 'rng_seed', 'stream'], params
    assert 'azg_train_gather_forms' in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(LIB), 'azg_train_gather_forms')
    assert len(_lib.lib().azg_train_gather_forms.argtypes) == 20


def test_gather_forms_refuses_bad_arguments_before_any_launch():
    """the refusals need no GPU: they return < 0 with the function's name (or the dispatch's message) before anything is launched"""
    from azg_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)                                   # (never dereferenced: every call below is refused or B == 0)
    p = ctypes.cast(buf, ctypes.c_void_p)
    rec, out = [p] * 5, [p] * 5

    def call(game=_lib.SPLENDOR, variant=2, rec=rec, first=p, end=p, streams=None, n=1, ids=p, B=1, out=out):
        return L.azg_train_gather_forms(game, variant, *rec, first, end, streams, n, ids, B, *out, 0, None)

    assert call(B=0) == 0 and call(B=0, rec=[None] * 5, first=None, end=None, ids=None, out=[None] * 5, n=0) == 0     # nothing to do
    assert call(B=-1) < 0 and b'azg_train_gather_forms' in L.azg_last_error()
    assert call(n=0) < 0 and b'azg_train_gather_forms' in L.azg_last_error()
    assert call(game=99, variant=0) < 0 and call(variant=7) < 0 and call(variant=7, B=0) < 0                           # unknown game / variant
    for k in range(5):
        assert call(rec=rec[:k] + [None] + rec[k + 1:]) < 0 and b'NULL' in L.azg_last_error()
        assert call(out=out[:k] + [None] + out[k + 1:]) < 0
    assert call(first=None) < 0 and call(end=None) < 0 and call(ids=None) < 0


# ---- the index arithmetic on CPU tensors ---------------------------------------------------------------------------------------------
def make_records(n, seed):
    r = np.random.default_rng(seed)
    return [r.integers(-128, 128, (n, S)).astype(np.int8), r.random((n, A), dtype=np.float32), r.standard_normal((n, P)).astype(np.float32),
            r.integers(0, 2, (n, A)).astype(np.uint8), r.standard_normal((n, P)).astype(np.float32)]


class Model:
    """the brute force: per iteration the list of (stream of the record, form) of its live rows, and the records' bytes by stream"""

    def __init__(self):
        self.iters, self.boards = [], {}

    def append(self, recs, counts, maxlen, stream0):
        rows = [(stream0 + t, k) for t, c in enumerate(counts) for k in range(c)]
        for t in range(len(counts)):
            self.boards[stream0 + t] = recs[0][t]
        total = len(rows)
        self.iters.append(rows if maxlen is None else rows[max(0, total - maxlen):])       # deque(maxlen): the LAST maxlen
        return len(self.iters[-1]), total

    def rows(self):
        return [x for it in self.iters for x in it]


def resolve(h):
    """what the kernel's contract gives for every virtual row: (stream of record g, k), g = the lowest record with row_end[g] > r"""
    first, end, stream = [x.numpy() for x in h.index_columns()]
    boards = h.record_columns()[0].numpy()
    assert (np.diff(end) >= 0).all(), 'row_end must be non-decreasing'
    out = []
    for r in range(h.n):
        g = int(np.searchsorted(end, r, side='right'))
        assert g < h.n_records and end[g] > r and (g == 0 or end[g - 1] <= r)
        out.append((int(stream[g]), int(r - first[g]), boards[g]))
    assert h.n_records == 0 or h.n == end[-1]                              # no record owns a row at or behind n
    return out


def agrees(h, m):
    got, want = resolve(h), m.rows()
    assert h.n == len(want) == sum(h.sizes) and h.sizes == [len(it) for it in m.iters] and h.n_records == sum(h.rec_sizes)
    assert [(s, k) for s, k, _ in got] == want
    assert all(np.array_equal(b, m.boards[s]) for s, _, b in got)
    return True


def test_append_maxlen_pop_and_truncate_against_the_brute_force():
    from azg_amd.history import CompactHistory
    h, m = CompactHistory(S, A, P, capacity=2), Model()
    assert h.n == 0 and len(h) == 0 and h.device_bytes() == 0 and h.row_bytes == S + 4 * A + 4 * P + A + 4 * P
    plan = [((3, 1, 4, 2), None), ((2, 5, 1, 3, 3), 5), ((4, 4), 100), ((1, 2, 3), 1), ((2, 2, 2), 2), ((5,), 3)]
    for i, (counts, maxlen) in enumerate(plan):
        recs = make_records(len(counts), i)
        s0 = 1000 * (i + 1)
        got = h.append_counted(GAME, recs, torch.tensor(counts, dtype=torch.int32), maxlen=maxlen, stream0=s0)
        assert got == m.append(recs, counts, maxlen, s0)
        assert agrees(h, m) and h.capacity >= h.n_records
    assert h.sizes == [10, 5, 8, 1, 2, 3] and h.rec_sizes == [4, 5, 2, 3, 3, 1] and len(h) == 6
    first, end, _ = [x.tolist() for x in h.index_columns()]
    assert first[4] == 10 - 9 and end[4:7] == [10, 10, 10]                 # iteration 2 kept its last 5 of 14: three records wholly cut,
    assert first[7] == 9 and end[7] == 12                                  # the cut inside the fourth (its first_row lies below the base 10)
    assert h.device_bytes() == 18 * (h.row_bytes + 24) < h.n * h.row_bytes
    # an empty iteration
    assert h.append_counted(GAME, make_records(0, 9), None) == (0, 0)
    m.iters.append([])
    assert agrees(h, m) and h.sizes[-1] == 0 and h.rec_sizes[-1] == 0
    # truncate_iteration keeps the FIRST rows: inside a record, at a record's edge, to nothing, and a no-op
    for i, rows in ((0, 7), (2, 4), (4, 0), (5, 9), (1, 5)):
        h.truncate_iteration(i, rows)
        m.iters[i] = m.iters[i][:rows]
        assert agrees(h, m)
    assert h.sizes == [7, 5, 4, 1, 0, 3, 0]
    # pop_oldest: the records move to the front (overlapping: 14 records over 4), the index is rebased
    ptr = h._bufs[0].data_ptr()
    while len(h):
        assert h.pop_oldest() == len(m.iters.pop(0))
        assert agrees(h, m) and h._bufs[0].data_ptr() == ptr
    assert h.n == 0 and h.n_records == 0 and h.device_bytes() == 0
    # an append behind pops lands on the new base
    recs = make_records(3, 50)
    assert h.append_counted(GAME, recs, torch.tensor([2, 2, 2]), maxlen=5, stream0=7) == m.append(recs, (2, 2, 2), 5, 7)
    assert agrees(h, m) and h.index_columns()[0].tolist() == [-1, 1, 3]


def test_valids_are_stored_as_bytes_and_boards_with_their_shape():
    from azg_amd.history import CompactHistory
    h = CompactHistory(S, A, P)
    c = make_records(4, 5)
    h.append_counted(GAME, [c[0].reshape(4, 3, 2), c[1], c[2], c[3].astype(bool), c[4]], torch.tensor([1, 1, 1, 1]))
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(h.record_columns(), c))
    assert [a.dtype for a in h.record_columns()] == [torch.int8, torch.float32, torch.float32, torch.uint8, torch.float32]
    assert h.index_columns()[2].tolist() == [0, 1, 2, 3]


def test_round_trip_through_the_record_file(tmp_path):
    from azg_amd.history import CompactHistory, DeviceHistory
    h = CompactHistory(S, A, P)
    for i, (counts, maxlen) in enumerate((((3, 1, 4), 6), ((), None), ((2, 2), None))):
        h.append_counted(GAME, make_records(len(counts), 30 + i), torch.tensor(counts, dtype=torch.int64) if counts else None, maxlen=maxlen,
                         stream0=(1 << 42) + 10 * i)
    path = str(tmp_path / 'checkpoint.records.npz')
    h.save_records(path)
    assert os.listdir(tmp_path) == ['checkpoint.records.npz']
    with np.load(path) as d:
        assert sorted(d.files) == sorted(['boards', 'pi', 'z', 'valids', 'q', 'first_row', 'row_end', 'stream', 'sizes', 'rec_sizes', 'game', 'rng_seed'])
        assert d['sizes'].tolist() == [6, 0, 4] and d['rec_sizes'].tolist() == [3, 0, 2] and int(d['rng_seed'][0]) == 77
    back = CompactHistory.load_records(path)
    assert (back.sizes, back.rec_sizes, back.n, back.n_records) == (h.sizes, h.rec_sizes, 10, 5)
    assert (back.game_id, back.variant, back.rng_seed) == (1, 2, 77) and back.widths == h.widths
    for a, b in zip(back.record_columns() + back.index_columns(), h.record_columns() + h.index_columns()):
        assert a.dtype == b.dtype and torch.equal(a, b)
    # a file of expanded columns is not a file of records
    d = DeviceHistory(S, A, P)
    d.append_columns(make_records(3, 1))
    cols = str(tmp_path / 'checkpoint.examples.npz')
    d.save_columns(cols)
    with pytest.raises(ValueError, match='not records'):
        CompactHistory.load_records(cols)


def test_the_rng_seed_and_the_game_are_fixed_by_the_first_append():
    from azg_amd.history import CompactHistory
    h = CompactHistory(S, A, P)
    assert h.rng_seed is None
    h.append_counted(GAME, make_records(2, 1), torch.tensor([1, 2]))
    assert (h.game_id, h.variant, h.rng_seed) == (1, 2, 77)
    with pytest.raises(ValueError, match='rng_seed'):
        h.append_counted(SimpleNamespace(GAME_ID=1, variant=2, rng_seed=78), make_records(2, 2), torch.tensor([1, 2]))
    with pytest.raises(ValueError, match='game'):
        h.append_counted(SimpleNamespace(GAME_ID=1, variant=3, rng_seed=77), make_records(2, 2), torch.tensor([1, 2]))
    assert h.sizes == [3] and h.n_records == 2                              # a refused append leaves the history as it was
    with pytest.raises(ValueError, match='CUDA'):
        h.append_records(GAME, make_records(2, 3) + [torch.zeros((2, 4), dtype=torch.int32)])
    with pytest.raises(ValueError, match='live rows'):
        h.rows(0, 4)


def test_the_host_trainer_refuses_a_compact_history():
    from azg_amd import train
    from azg_amd.history import CompactHistory
    h = CompactHistory(S, A, P)
    h.append_counted(GAME, make_records(2, 1), torch.tensor([1, 2]))
    with pytest.raises(ValueError, match='device_batches'):
        train.train(torch.nn.Linear(1, 1), h, batch_size=1, device='cpu')
    with pytest.raises(ValueError, match='CUDA'):                           # (device_batches has no CPU form, compact or not)
        train.train(torch.nn.Linear(1, 1), h, batch_size=1, device='cpu', device_batches=True)


# ---- Coach ---------------------------------------------------------------------------------------------------------------------------
class StubNet:
    """the NeuralNet surface Coach.__init__ touches"""

    def __init__(self, game=None, args=None):
        self.game, self.args, self.nnet = game, dict(args or {}), None

    def save_checkpoint(self, *a, **kw):
        pass


def make_coach(folder, kind, device_batches=True, **kw):
    from azg_amd.coach import Coach
    game = SimpleNamespace(S=S, A=A, P=P, device='cpu', GAME_ID=1, variant=2, rng_seed=77)
    logs = []
    args = dict(numEps=4, checkpoint=str(folder), **kw)
    return Coach(game, StubNet(game, dict(device_batches=device_batches)), args, n_games=4, log=logs.append, dist=False,
                 device_history=kind), logs


def test_coach_selects_the_compact_history_and_checks_its_arguments(tmp_path):
    from azg_amd.history import CompactHistory, DeviceHistory
    c, _ = make_coach(tmp_path, 'compact')
    assert isinstance(c.device_history, CompactHistory) and c.device_history.widths == (S, A, P, A, P)
    c, _ = make_coach(tmp_path, None, device_history='compact', examples_file='records')             # args.device_history
    assert isinstance(c.device_history, CompactHistory)
    c, _ = make_coach(tmp_path, True)                                                                # True keeps today's history
    assert type(c.device_history) is DeviceHistory
    c, _ = make_coach(tmp_path, None, device_batches=False)
    assert c.device_history is None
    with pytest.raises(ValueError, match='device_batches'):
        make_coach(tmp_path, 'compact', device_batches=False)
    with pytest.raises(ValueError, match='examples_file'):
        make_coach(tmp_path, 'compact', examples_file='pickle')
    with pytest.raises(ValueError, match='examples_file'):
        make_coach(tmp_path, True, examples_file='records')                                          # records are the compact history's file
    with pytest.raises(ValueError, match='compact'):
        make_coach(tmp_path, 'dense')


def test_coach_saves_and_resumes_records_and_refuses_expanded_rows(tmp_path):
    import pickle
    from azg_amd.history import CompactHistory
    src = tmp_path / 'src'
    c, _ = make_coach(src, 'compact', examples_file='records')
    for i, counts in enumerate(((3, 1, 4), (2, 2), (1, 5))):
        c.device_history.append_counted(c.game, make_records(len(counts), 40 + i), torch.tensor(counts), stream0=(1 << 42) + 3 * i)
        c._ref_iters.append(None)
    c.n_selfplay_waves, c._sym_stream = 3, 8
    c.saveTrainExamples(iterations_done=3)
    assert sorted(os.listdir(src)) == ['azg_state.json', 'checkpoint.records.npz']
    fresh, logs = make_coach(tmp_path / 'a', 'compact', examples_file='records', load_folder_file=[str(src), 'best.pt'], numItersHistory=2,
                             maxlenOfQueue=5)
    fresh.loadTrainExamples()
    h = fresh.device_history
    assert logs == [] and isinstance(h, CompactHistory) and h.sizes == [4, 5] and h.rec_sizes == [2, 2] and fresh._ref_iters == [None, None]
    assert (fresh.n_selfplay_waves, fresh.iter_base, fresh._sym_stream) == (3, 3, 8)
    assert h.index_columns()[0].tolist() == [0, 2, 4, 5] and h.index_columns()[1].tolist() == [2, 4, 5, 9]
    assert h.index_columns()[2].tolist() == [(1 << 42) + 3, (1 << 42) + 4, (1 << 42) + 6, (1 << 42) + 7]
    # no file: said, not raised
    none, logs = make_coach(tmp_path / 'b', 'compact', load_folder_file=[str(tmp_path / 'nowhere'), 'best.pt'])
    none.loadTrainExamples()
    assert len(logs) == 1 and 'not found' in logs[0] and none.device_history.n == 0
    # a reference file (expanded rows) cannot become records
    ref = tmp_path / 'ref'
    os.makedirs(ref)
    with open(ref / 'checkpoint.examples', 'wb') as f:
        pickle.dump([], f)
    bad, _ = make_coach(tmp_path / 'c', 'compact', load_folder_file=[str(ref), 'best.pt'])
    with pytest.raises(ValueError, match='records'):
        bad.loadTrainExamples()
    # records written with another rng_seed would expand to other rows
    other, _ = make_coach(tmp_path / 'd', 'compact', examples_file='records', load_folder_file=[str(src), 'best.pt'])
    other.game.rng_seed = 78
    with pytest.raises(ValueError, match='rng_seed'):
        other.loadTrainExamples()
