"""GPU: Coach(device_history=True) -- the example history as device columns (azg_amd/history.py), filled in place by azg_examples_expand
and read in place by the device-batch trainer.  Splendor-2p with the shipped V80 weights at the scale of
tests/test_gpu_coach.py::test_coach_learn_two_iterations (8 simulations, 16 episodes, 32 games, batch 32).  The default path of the same
commit is the yardstick: the same seed gives the same self-play, so the device history must hold, row for row and bit for bit, what the
default path's deque holds, and the file it writes must decode to its own rows."""
import copy
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 3


class Args(dict):
    __getattr__ = dict.get


def make_args(folder, **kw):
    a = Args(numMCTSSims=8, cpuct=0.8, fpu=0.0593, universes=3, forced_playouts=False, dirichletAlpha=0.3, prob_fullMCTS=1.0,
             ratio_fullMCTS=5, temperature=[1.25, 0.8, 1.0], tempThreshold=6, numIters=1, numEps=16, numItersHistory=1,
             maxlenOfQueue=100000, learn_rate=1e-3, batch_size=32, epochs=1, q_weight=0.5, arenaCompare=4, updateThreshold=0.6,
             checkpoint=str(folder), seed=SEED, device_batches=True)
    a.update(kw)
    return a


def make_module():
    import torch
    from azg_amd.train import SplendorV80Module
    z = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'weights_splendor2_v80.npz'))
    m = SplendorV80Module(2)
    m.load_state_dict({k[3:]: torch.as_tensor(z[k]) for k in z.files if k.startswith('sd/')})
    return m


def make_coach(folder, device_history=True, **kw):
    from azg_amd import games
    from azg_amd.coach import Coach
    logs = []
    c = Coach(games.SplendorGame(2), make_module(), make_args(folder, **kw), n_games=32, node_capacity=1024, log=logs.append,
              device_history=device_history)
    return c, logs


def decoded(iteration):
    """a deque / list of (possibly compressed) examples -> the five columns as numpy arrays, in order"""
    from azg_amd.nnet_wrapper import decode_examples
    cols = decode_examples(list(iteration))
    return [cols[0].astype(np.int8), cols[1].astype(np.float32), cols[2].astype(np.float32), cols[3].astype(np.uint8), cols[4].astype(np.float32)]


def same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
                                    for x, y in zip(a, b))


def host(cols):
    return [np.ascontiguousarray(c.cpu().numpy()) for c in cols]


@pytest.fixture(scope='module')
def default_iteration(tmp_path_factory):
    """iteration 1 of the default path: its deque, decoded and unshuffled"""
    c, _ = make_coach(tmp_path_factory.mktemp('default'), device_history=False)
    assert c.device_history is None
    it = c.executeEpisodes()
    return decoded(it), c._sym_stream


@pytest.fixture(scope='module')
def one_iteration(tmp_path_factory):
    """learn() with numIters = 1 on the device history; the weights are taken right behind nnet.train (the arena gate may put the old
    ones back afterwards)"""
    import torch
    folder = tmp_path_factory.mktemp('one')
    c, logs = make_coach(folder)
    initial = copy.deepcopy(c.nnet.nnet)
    trained = {}
    inner = c.nnet.train

    def spy(examples, **kw):
        out = inner(examples, **kw)
        torch.cuda.synchronize()
        trained.update({k: v.detach().cpu().clone() for k, v in c.nnet.nnet.state_dict().items()})
        trained['__cols__'] = examples
        return out

    c.nnet.train = spy
    res = c.learn()
    return dict(coach=c, logs=logs, initial=initial, trained=trained, results=res, folder=str(folder))


@pytest.fixture(scope='module')
def two_iterations(tmp_path_factory):
    """numIters = 2 with numItersHistory = 1: the first iteration is popped, the second moves to the front"""
    folder = tmp_path_factory.mktemp('two')
    c, logs = make_coach(folder, numIters=2)
    res = c.learn()
    return dict(coach=c, logs=logs, results=res, folder=str(folder))


def test_construction_needs_device_batches(tmp_path):
    with pytest.raises(ValueError, match='device_batches'):
        make_coach(tmp_path, device_batches=False)
    with pytest.raises(ValueError, match='examples_file'):
        make_coach(tmp_path, examples_file='pickle')
    c, _ = make_coach(tmp_path, device_history=None, device_batches=False)            # the default stays the default
    assert c.device_history is None
    from azg_amd.coach import Coach
    from azg_amd import games
    c = Coach(games.SplendorGame(2), make_module(), make_args(tmp_path, device_history=True), n_games=32)      # args.device_history
    assert c.device_history is not None


def test_history_equals_the_file_the_same_run_wrote(two_iterations):
    from azg_amd import formats
    c = two_iterations['coach']
    h = c.device_history
    assert len(two_iterations['results']) == 2 and all(r['examples'] > 64 for r in two_iterations['results'])
    assert len(h) == 1 and h.n == h.sizes[0] == two_iterations['results'][1]['examples']            # iteration 1 was popped
    assert c.trainExamplesHistory == []                                                            # nothing is decoded on the host
    import pickle
    with open(os.path.join(two_iterations['folder'], 'checkpoint.examples'), 'rb') as f:
        raw = pickle.load(f)
    assert [len(it) for it in raw] == h.sizes and raw[0].maxlen == 100000 and isinstance(raw[0][0], bytes)
    hist = formats.load_train_examples(os.path.join(two_iterations['folder'], 'checkpoint.examples'))
    assert hist[0][0][0].shape == (56, 7) and hist[0][0][3].dtype == bool
    assert same_bits(host(h.columns()), decoded(raw[0]))
    assert all(t.is_contiguous() and t.data_ptr() == b.data_ptr() for t, b in zip(h.columns(), h._bufs))


def test_iteration_one_equals_the_default_path(one_iteration, default_iteration):
    c = one_iteration['coach']
    want, sym_stream = default_iteration
    assert len(c.device_history) == 1 and c._sym_stream == sym_stream > 0
    got = host(c.device_history.iteration_columns(0))
    assert len(got[0]) == len(want[0]) > 64
    assert same_bits(got, want)
    # the Dirichlet advice of Coach.py:169-176 from the new rows' valids
    avg = float(want[3].sum()) / len(want[3])
    said = [m for m in one_iteration['logs'] if 'valid moves per state' in m]
    if 1 / 1.5 < 0.3 / (10 / avg) < 1.5:
        assert said == []
    else:
        assert said == ['There are about %.1f valid moves per state, so I advise to set dirichlet to %.1f instead' % (avg, 10 / avg)]


def test_training_reads_the_history_in_place(one_iteration):
    import torch
    from azg_amd import train
    c, trained = one_iteration['coach'], one_iteration['trained']
    cols = trained['__cols__']
    assert all(a.data_ptr() == b.data_ptr() and a.shape == b.shape for a, b in zip(cols, c.device_history.columns()))
    assert one_iteration['results'][0]['examples'] == c.device_history.n
    m = copy.deepcopy(one_iteration['initial'])
    train.train(m, c.device_history.iteration_columns(0), learn_rate=1e-3, batch_size=32, epochs=1, q_weight=0.5, device=str(c.game.device),
                seed=SEED + 1, device_batches=True)
    torch.cuda.synchronize()
    sd = m.state_dict()
    assert set(sd) == set(trained) - {'__cols__'}
    for k, v in sd.items():
        assert torch.equal(v.detach().cpu(), trained[k]), k
    assert any(not torch.equal(v.detach().cpu(), one_iteration['initial'].state_dict()[k].cpu()) for k, v in sd.items())     # (it did train)


def test_maxlen_keeps_the_last_rows_and_says_so(tmp_path, default_iteration):
    want, _ = default_iteration
    maxlen = 50
    assert len(want[0]) > maxlen
    c, logs = make_coach(tmp_path, maxlenOfQueue=maxlen, profile=True)                # (profile: learn() returns behind the self-play)
    c.learn()
    h = c.device_history
    assert h.sizes == [maxlen] and h.n == maxlen
    assert same_bits(host(h.columns()), [w[-maxlen:] for w in want])
    assert [m for m in logs if m.startswith('saturation of elements in iterationTrainExamples')]
    # a second iteration lands behind the first, which stays as it was
    before = host(h.columns())
    kept, total = c.executeEpisodes(to_history=True)
    assert (kept, h.sizes, h.n) == (maxlen, [maxlen, maxlen], 2 * maxlen) and total > maxlen
    assert same_bits(host(h.iteration_columns(0)), before)


@pytest.mark.parametrize('kind', ['reference', 'columns'])
def test_resume(two_iterations, tmp_path, kind):
    c = two_iterations['coach']
    folder = two_iterations['folder']
    if kind == 'columns':
        c.args['examples_file'] = 'columns'
        try:
            c.saveTrainExamples(iterations_done=2)
        finally:
            c.args['examples_file'] = 'reference'
        assert os.path.isfile(os.path.join(folder, 'checkpoint.examples.npz'))
    with open(os.path.join(folder, 'azg_state.json')) as f:
        st = json.load(f)
    assert st == dict(selfplay_waves=2, iterations_done=2, sym_stream=c._sym_stream)
    fresh, logs = make_coach(tmp_path, examples_file=kind, load_folder_file=[folder, 'best.pt'])
    fresh.loadTrainExamples()
    assert logs == []
    assert fresh.device_history.sizes == c.device_history.sizes
    assert same_bits(host(fresh.device_history.columns()), host(c.device_history.columns()))
    assert (fresh.n_selfplay_waves, fresh.iter_base, fresh._sym_stream) == (2, 2, c._sym_stream)
    # the same trimming as the default path: maxlenOfQueue drops from the END of a loaded iteration
    short, _ = make_coach(tmp_path, examples_file=kind, load_folder_file=[folder, 'best.pt'], maxlenOfQueue=40)
    short.loadTrainExamples()
    assert short.device_history.sizes == [40]
    assert same_bits(host(short.device_history.columns()), [x[:40] for x in host(c.device_history.columns())])
    # ... and what was loaded can be saved again in the reference's layout
    short.args['checkpoint'] = str(tmp_path)
    short.saveTrainExamples(iterations_done=2)
    if kind == 'reference':
        import pickle
        with open(os.path.join(str(tmp_path), 'checkpoint.examples'), 'rb') as f:
            again = pickle.load(f)
        assert same_bits(decoded(again[0]), host(short.device_history.columns()))
