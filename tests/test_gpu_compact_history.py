"""GPU: Coach(device_history='compact') -- the example history as records (history.CompactHistory), their forms computed by the gather of
every training batch (azg_train_gather_forms).  The Splendor-2p Coach of tests/test_gpu_device_history.py (8 simulations, 16 episodes,
32 games, batch 32) on the same seed, once with device_history=True and once with 'compact': the same self-play, so the compact
history's virtual rows must be, bit for bit, the rows of the expanded history -- after one iteration, under a maxlenOfQueue smaller than
the iteration, and after a second iteration that pops the first; training on either must give the same per-step losses and the same
weights, eagerly and with graph_step; the files it writes must decode to its rows; and its device bytes are those of its records.
One The Little Prince (3 players) append covers the games whose forms draw."""
import copy
import os
import pickle

import numpy as np
import pytest

from test_gpu_device_history import SEED, decoded, host, make_coach, same_bits

pytestmark = pytest.mark.gpu


def learn_one(folder, kind, **kw):
    """learn() with numIters = 1: the Coach, what nnet.train returned (the per-step losses) and the weights right behind it"""
    import torch
    c, logs = make_coach(folder, device_history=kind, **kw)
    initial = copy.deepcopy(c.nnet.nnet)
    seen = {}
    inner = c.nnet.train

    def spy(examples, **k):
        out = inner(examples, **k)
        torch.cuda.synchronize()
        seen.update(losses=list(out), examples=examples, weights={n: v.detach().cpu().clone() for n, v in c.nnet.nnet.state_dict().items()})
        return out

    c.nnet.train = spy
    res = c.learn()
    return dict(coach=c, logs=logs, initial=initial, results=res, folder=str(folder), **seen)


def release(coaches):
    """close the self-play engines now (their forests, streams and hardware queues), not whenever the collector finds the cycles"""
    import gc
    for c in coaches:
        if c.engine is not None:
            c.engine.close()
            c.engine = None
    gc.collect()


@pytest.fixture(scope='module')
def pair(tmp_path_factory):
    """one iteration of learn() on either history, the same seed"""
    out = {kind: learn_one(tmp_path_factory.mktemp('one_%s' % kind), kind) for kind in (True, 'compact')}
    yield out
    release([v['coach'] for v in out.values()])


@pytest.fixture(scope='module')
def pair_two(tmp_path_factory):
    """numIters = 2 with numItersHistory = 1: the first iteration is popped"""
    out = {}
    for kind in (True, 'compact'):
        c, logs = make_coach(tmp_path_factory.mktemp('two_%s' % kind), device_history=kind, numIters=2)
        out[kind] = dict(coach=c, logs=logs, results=c.learn(), folder=c.args['checkpoint'])
    yield out
    release([v['coach'] for v in out.values()])


def test_one_iteration_holds_the_rows_of_the_expanded_history(pair):
    from azg_amd.history import CompactHistory, DeviceHistory
    d, c = pair[True]['coach'].device_history, pair['compact']['coach'].device_history
    assert type(d) is DeviceHistory and type(c) is CompactHistory
    assert c.sizes == d.sizes and c.n == d.n > 64 and len(c) == 1
    assert c.n_records == c.rec_sizes[0] < c.n                                          # fewer records than rows
    assert same_bits(host(c.rows(0, c.n)), host(d.columns()))
    assert same_bits(host(c.rows(5, 37)), [x[5:37] for x in host(d.columns())])          # a range that starts inside a record
    assert pair['compact']['coach']._sym_stream == pair[True]['coach']._sym_stream > 0
    assert pair['compact']['results'][0]['examples'] == pair[True]['results'][0]['examples'] == d.n
    assert pair['compact']['logs'] == pair[True]['logs']                                 # the Dirichlet advice included, word for word
    # bytes: the records and 24 bytes of index each, against the expanded rows
    row = 392 + 4 * 81 + 4 * 2 + 81 + 4 * 2
    assert c.row_bytes == row and c.device_bytes() == c.n_records * (row + 24) < c.n * row
    # the trainer was given the history itself, not columns
    assert pair['compact']['examples'] is c


def test_training_gives_the_same_losses_and_weights(pair):
    import torch
    a, b = pair[True], pair['compact']
    assert len(a['losses']) == len(b['losses']) >= 2 and a['losses'] == b['losses']      # per step, bit for bit (floats from one f64 buffer)
    assert set(a['weights']) == set(b['weights'])
    for k, v in a['weights'].items():
        assert torch.equal(v, b['weights'][k]), k
    assert any(not torch.equal(v, a['initial'].state_dict()[k].cpu()) for k, v in a['weights'].items())      # (it did train)


@pytest.mark.parametrize('mode', ['eager_device_optimizer', 'graph_step'])
def test_the_device_optimiser_and_the_graph_step_read_the_same_batches(pair, mode):
    import torch
    from azg_amd import train
    d, c = pair[True]['coach'].device_history, pair['compact']['coach'].device_history
    kw = dict(learn_rate=1e-3, batch_size=32, epochs=1, q_weight=0.5, device=str(d.device), seed=SEED + 9, device_batches=True,
              device_optimizer=True, graph_step=mode == 'graph_step')
    out = []
    for examples in (d.columns(), c):
        m, info = copy.deepcopy(pair[True]['initial']), {}
        losses = train.train(m, examples, info=info, **kw)
        torch.cuda.synchronize()
        out.append((losses, {k: v.detach().cpu() for k, v in m.state_dict().items()}, info))
    (la, wa, ia), (lb, wb, ib) = out
    steps = d.n // 32
    assert len(la) == len(lb) == steps and la == lb
    assert ia == ib and ia['graph_replays'] == (steps - 1 if mode == 'graph_step' else 0)
    for k, v in wa.items():
        assert torch.equal(v, wb[k]), k


def test_batch_ids_name_virtual_rows(pair):
    """batch_ids on either history: the same ids give the same steps (two epochs, torch's optimiser); an id at n is refused"""
    from azg_amd import train
    d, c = pair[True]['coach'].device_history, pair['compact']['coach'].device_history
    kw = dict(learn_rate=1e-3, batch_size=32, epochs=2, q_weight=0.5, device=str(d.device), device_batches=True)
    ids = np.random.default_rng(3).integers(0, d.n, (2 * (d.n // 32), 32))
    got = [train.train(copy.deepcopy(pair[True]['initial']), e, batch_ids=ids, **kw) for e in (d.columns(), c)]
    assert len(got[0]) == len(ids) and got[0] == got[1]
    with pytest.raises(ValueError, match='outside'):
        train.train(copy.deepcopy(pair[True]['initial']), c, batch_ids=np.full(ids.shape, c.n), **kw)


def test_the_reference_file_decodes_to_the_same_rows(pair):
    c = pair['compact']['coach']
    with open(os.path.join(pair['compact']['folder'], 'checkpoint.examples'), 'rb') as f:
        raw = pickle.load(f)
    with open(os.path.join(pair[True]['folder'], 'checkpoint.examples'), 'rb') as f:
        want = pickle.load(f)
    assert [len(it) for it in raw] == c.device_history.sizes and raw[0].maxlen == 100000 and isinstance(raw[0][0], bytes)
    assert list(raw[0]) == list(want[0])                                                # the very bytes the expanded history wrote
    assert same_bits(decoded(raw[0]), host(c.device_history.rows(0, c.device_history.n)))
    # ... and the column file
    c.args['examples_file'] = 'columns'
    try:
        c.saveTrainExamples(iterations_done=1)
    finally:
        c.args['examples_file'] = 'reference'
    with np.load(os.path.join(pair['compact']['folder'], 'checkpoint.examples.npz')) as z:
        assert z['sizes'].tolist() == c.device_history.sizes
        assert same_bits([z[k] for k in ('boards', 'pi', 'z', 'valids', 'q')], host(pair[True]['coach'].device_history.columns()))


def test_a_second_iteration_pops_the_first(pair_two):
    d, c = pair_two[True]['coach'].device_history, pair_two['compact']['coach'].device_history
    assert len(c) == len(d) == 1 and c.sizes == d.sizes and c.n == d.n > 64 and len(c.rec_sizes) == 1 and c.n_records == c.rec_sizes[0]
    assert int(c.index_columns()[0][0]) == 0 and int(c.index_columns()[1][-1]) == c.n    # rebased: the survivor starts at row 0
    assert same_bits(host(c.rows(0, c.n)), host(d.columns()))
    assert pair_two['compact']['results'] == pair_two[True]['results']                   # examples, arena tallies, accepted: all equal
    assert pair_two['compact']['logs'] == pair_two[True]['logs']


def test_maxlen_smaller_than_one_iteration(tmp_path, pair):
    full = host(pair[True]['coach'].device_history.columns())
    maxlen = 50
    got = {}
    for kind in (True, 'compact'):
        c, logs = make_coach(tmp_path / str(kind), device_history=kind, maxlenOfQueue=maxlen, profile=True)
        c.learn()
        got[kind] = (c, logs, c.executeEpisodes(to_history=True))                        # a second iteration behind the cut one
    d, c = got[True][0].device_history, got['compact'][0].device_history
    assert got['compact'][2] == got[True][2] and got[True][2][0] == maxlen < got[True][2][1]           # (kept, total)
    assert c.sizes == d.sizes == [maxlen, maxlen] and c.n == 2 * maxlen
    assert same_bits(host(c.rows(0, c.n)), host(d.columns()))
    assert same_bits(host(c.iteration_columns(0)), [w[-maxlen:] for w in full])
    assert int(c.index_columns()[0][:c.rec_sizes[0]].min()) < 0                          # first_row keeps its true value below the base
    assert got['compact'][1] == got[True][1] and [m for m in got['compact'][1] if m.startswith('saturation')]
    assert c.device_bytes() == c.n_records * (c.row_bytes + 24)
    release([got[True][0], got['compact'][0]])


def test_records_save_load_and_resume(pair_two, tmp_path):
    import json
    from azg_amd.history import CompactHistory
    c = pair_two['compact']['coach']
    folder = pair_two['compact']['folder']
    c.args['examples_file'] = 'records'
    try:
        c.saveTrainExamples(iterations_done=2)
    finally:
        c.args['examples_file'] = 'reference'
    path = os.path.join(folder, 'checkpoint.records.npz')
    h = c.device_history
    back = CompactHistory.load_records(path, device=h.device)
    assert (back.sizes, back.rec_sizes, back.game_id, back.variant, back.rng_seed) == (h.sizes, h.rec_sizes, h.game_id, h.variant, h.rng_seed)
    assert same_bits(host(back.record_columns() + back.index_columns()), host(h.record_columns() + h.index_columns()))
    assert same_bits(host(back.rows(0, back.n)), host(h.rows(0, h.n)))
    with open(os.path.join(folder, 'azg_state.json')) as f:
        assert json.load(f) == dict(selfplay_waves=2, iterations_done=2, sym_stream=c._sym_stream)
    fresh, logs = make_coach(tmp_path, device_history='compact', examples_file='records', load_folder_file=[folder, 'best.pt'])
    fresh.loadTrainExamples()
    assert logs == [] and fresh.device_history.sizes == h.sizes
    assert same_bits(host(fresh.device_history.rows(0, h.n)), host(h.rows(0, h.n)))
    assert (fresh.n_selfplay_waves, fresh.iter_base, fresh._sym_stream) == (2, 2, c._sym_stream)
    # maxlenOfQueue drops from the END of a loaded iteration
    short, _ = make_coach(tmp_path, device_history='compact', examples_file='records', load_folder_file=[folder, 'best.pt'], maxlenOfQueue=40)
    short.loadTrainExamples()
    assert short.device_history.sizes == [40]
    assert same_bits(host(short.device_history.rows(0, 40)), [x[:40] for x in host(h.rows(0, h.n))])
    # the reference file of the same folder is expanded rows: not records
    os.remove(path)
    with pytest.raises(ValueError, match='records'):
        fresh.loadTrainExamples()


def test_the_little_prince_draws_the_same_forms(golden_dir):
    """append_records + rows against DeviceHistory on the same drained records: the canonical order, the streams and the draws"""
    import torch
    from azg_amd import games
    from azg_amd.history import CompactHistory, DeviceHistory
    from test_gpu_examples_expand import records
    g = games.TLPGame(num_players=3, rng_seed=1234)
    recs = records(golden_dir, 'tlp3', g, limit=40)
    n = len(recs[0])
    r = np.random.default_rng(2)
    meta = np.stack([r.integers(0, 3, n), r.integers(0, 4, n), r.permutation(n), np.zeros(n)], axis=1).astype(np.int32)      # stream, game, ply
    dev = [torch.from_numpy(x).to(g.device) for x in recs + [meta]]
    d, c = DeviceHistory(g.S, g.A, g.P, device=g.device), CompactHistory(g.S, g.A, g.P, device=g.device)
    for s0, maxlen in (((1 << 42) + 5, None), ((1 << 42) + 5 + n, 70)):
        assert c.append_records(g, dev, maxlen=maxlen, stream0=s0) == d.append_records(g, dev, maxlen=maxlen, stream0=s0)
    assert c.sizes == d.sizes and c.sizes[1] == 70 and c.n_records == 2 * n
    assert same_bits(host(c.rows(0, c.n)), host(d.columns()))
    assert same_bits(host(c.iteration_columns(1)), host(d.iteration_columns(1)))
    other = games.TLPGame(num_players=3, rng_seed=99)
    with pytest.raises(ValueError, match='rng_seed'):
        c.append_records(other, dev)
