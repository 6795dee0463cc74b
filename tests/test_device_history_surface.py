"""CPU-only: the surface of the device-resident example history -- azg_examples_expand declared in include/azg.h, exported by the built
library and bound by _lib.py; history.DeviceHistory's bookkeeping on CPU tensors (append, pop, growth, the contiguous prefix, the round
trips through the reference's layout and through the column file, a checkpoint.examples written by the reference); Coach's new trailing
keyword; and the code-object notes of the k_examples_* kernels (csrc/examples.hip.h), read as
tests/test_train_adamw_resources.py reads them.

Measured build (VGPRs; bound = the next multiple of 16 above): k_examples_expand -- Splendor 2 / 3 / 4: 41 / 34 / 41 (48), Santorini 1 / 11:
28 / 33 (32 / 48), Azul 22 (32), Abalone 31 (32), Minivilles 10 (16); k_examples_expand_built -- The Little Prince 3 / 4 / 5: 51 / 82 / 145
(64 / 96 / 160), Botanik 284 (288), Akropolis 2 / 3 / 4: 78 / 96 / 62 (80 / 112 / 64), Smallworld 24 (32).  LDS equals that of the
k_env_symmetries* kernel of the same game in every case.  (The Little Prince's kernels are free of scratch because TLPDev::sym_build keeps
the lists it shuffles as 4-bit entries of a 64-bit word and copies the mapped rows directly: with private arrays indexed at run time
they carried 256 / 288 / 320 B per lane.)"""
import ctypes
import inspect
import os
import pickle
import re
import zlib

import numpy as np
import pytest
import torch

from test_kernel_resources import LIB, LLVM, kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
_BUILT = os.path.exists(os.path.join(LLVM, 'llvm-readelf')) and os.path.exists(LIB)

# kernel fragment -> VGPR bound (the next multiple of 16 above the measured build, module docstring)
VGPR_BOUNDS = {
    'k_examples_expand<azg::SplendorDev<2> >': 48, 'k_examples_expand<azg::SplendorDev<3> >': 48, 'k_examples_expand<azg::SplendorDev<4> >': 48,
    'k_examples_expand<azg::SantoriniDev<1> >': 32, 'k_examples_expand<azg::SantoriniDev<11> >': 48, 'k_examples_expand<azg::AzulDev>': 32,
    'k_examples_expand<azg::AbaloneDevT<false> >': 32, 'k_examples_expand<azg::AbaloneDevT<true> >': 32,
    'k_examples_expand<azg::MinivillesDev<2> >': 16, 'k_examples_expand<azg::MinivillesDev<3> >': 16, 'k_examples_expand<azg::MinivillesDev<4> >': 16,
    'k_examples_expand_built<azg::TLPDev<3> >': 64, 'k_examples_expand_built<azg::TLPDev<4> >': 96, 'k_examples_expand_built<azg::TLPDev<5> >': 160,
    'k_examples_expand_built<azg::BotanikDev>': 288,
    'k_examples_expand_built<azg::AkropolisDev<2> >': 80, 'k_examples_expand_built<azg::AkropolisDev<3> >': 112, 'k_examples_expand_built<azg::AkropolisDev<4> >': 64,
    'k_examples_expand_built<azg::SmallworldDev<2> >': 32, 'k_examples_expand_built<azg::SmallworldDev<3> >': 32, 'k_examples_expand_built<azg::SmallworldDev<4> >': 32,
}


def test_examples_expand_is_declared_exported_and_bound():
    from azg_amd import _lib
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'azg.h')).read(), flags=re.S)
    m = re.search(r'\bint\s+azg_examples_expand\s*\(([^;]*)\)\s*;', h)
    assert m, 'include/azg.h does not declare azg_examples_expand'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    assert [p.split()[-1].lstrip('*') for p in params] == [
        'game', 'variant', 'states_dev', 'pi_dev', 'z_dev', 'valids_dev', 'q_dev', 'n', 'order_dev', 'first_row_dev', 'row_begin', 'row_end',
        'out_states_dev', 'out_pi_dev', 'out_z_dev', 'out_valids_dev', 'out_q_dev', 'out_count_dev', 'rng_seed', 'stream0', 'stream'], params
    assert 'azg_examples_expand' in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(LIB), 'azg_examples_expand')
    assert len(_lib.lib().azg_examples_expand.argtypes) == 21


def test_examples_expand_refuses_bad_arguments_before_any_launch():
    """the refusals need no GPU: they return < 0 with the function's name (or the dispatch's message) before anything is launched"""
    from azg_amd import _lib
    L = _lib.lib()
    null = [None] * 5
    buf = ctypes.create_string_buffer(64)                                   # (never dereferenced: every call below is refused or n == 0)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ins = [p] * 5
    assert L.azg_examples_expand(_lib.SPLENDOR, 2, *null, 0, None, None, 0, 0, *null, None, 0, 0, None) == 0        # n == 0: nothing to do
    assert L.azg_examples_expand(_lib.SPLENDOR, 2, *null, 1, None, None, 0, 0, *null, p, 0, 0, None) < 0            # null inputs, n > 0
    assert b'azg_examples_expand' in L.azg_last_error()
    assert L.azg_examples_expand(_lib.SPLENDOR, 2, *ins, 1, None, None, 0, 0, *null, None, 0, 0, None) < 0          # no out_count
    assert L.azg_examples_expand(_lib.SPLENDOR, 7, *ins, 0, None, None, 0, 0, *null, p, 0, 0, None) < 0             # unknown variant
    assert L.azg_examples_expand(99, 0, *ins, 0, None, None, 0, 0, *null, p, 0, 0, None) < 0                        # unknown game
    assert L.azg_examples_expand(_lib.SPLENDOR, 2, *ins, 0, None, None, 5, 4, *null, p, 0, 0, None) < 0             # row_end < row_begin
    assert b'row_end' in L.azg_last_error()
    assert L.azg_examples_expand(_lib.SPLENDOR, 2, *ins, 1, None, p, 0, 4, *null, p, 0, 0, None) < 0                # write pass without columns


# ---- DeviceHistory on CPU tensors ---------------------------------------------------------------------------------------------------
S, A, P = 6, 5, 2


def make_cols(n, seed):
    r = np.random.default_rng(seed)
    return [r.integers(-128, 128, (n, S)).astype(np.int8), r.random((n, A), dtype=np.float32), r.standard_normal((n, P)).astype(np.float32),
            r.integers(0, 2, (n, A)).astype(np.uint8), r.standard_normal((n, P)).astype(np.float32)]


def cat(parts):
    return [np.concatenate([p[k] for p in parts]) for k in range(5)]


def same(h, want):
    got = h.columns()
    assert all(g.is_contiguous() and g.shape[0] == h.n == sum(h.sizes) for g in got)
    assert [g.dtype for g in got] == [torch.int8, torch.float32, torch.float32, torch.uint8, torch.float32]
    return all(np.array_equal(g.numpy(), w) for g, w in zip(got, want))


def test_append_pop_growth_and_the_contiguous_prefix():
    from azg_amd.history import DeviceHistory
    h = DeviceHistory(S, A, P, capacity=4)
    its = [make_cols(n, i) for i, n in enumerate((3, 7, 0, 5, 2))]
    assert h.capacity == 4 and h.n == 0 and len(h) == 0 and same(h, cat([make_cols(0, 0)]))
    for j, it in enumerate(its):
        assert h.append_columns(it) == len(it[0])
        assert same(h, cat(its[:j + 1])) and h.capacity >= h.n                    # growth copied the live rows
    assert h.sizes == [3, 7, 0, 5, 2] and h.capacity >= 17
    ptrs = [b.data_ptr() for b in h.columns()]
    for j in range(1, 5):                                                        # overlapping move (7 + 5 + 2 rows over 3), empty iteration, ...
        h.pop_oldest()
        assert h.sizes == [3, 7, 0, 5, 2][j:] and same(h, cat(its[j:]))
        assert [b.data_ptr() for b in h.columns()] == ptrs                       # the prefix starts where the buffers start
    for k, (a, w) in enumerate(zip(h.iteration_columns(-1), its[4])):
        assert np.array_equal(a.numpy(), w), k
    h.pop_oldest()
    assert h.n == 0 and len(h) == 0
    # doubling: one row more than the capacity reallocates to at least twice the capacity, never less than what is needed
    h = DeviceHistory(S, A, P, capacity=8)
    h.append_columns(make_cols(8, 1))
    h.append_columns(make_cols(1, 2))
    assert h.capacity >= 16 and same(h, cat([make_cols(8, 1), make_cols(1, 2)]))
    h.append_columns(make_cols(100, 3))
    assert h.capacity >= 109 and h.n == 109
    # valids given as bool, boards given with their board shape
    h = DeviceHistory(S, A, P)
    c = make_cols(4, 5)
    h.append_columns([c[0].reshape(4, 3, 2), c[1], c[2], c[3].astype(bool), c[4]])
    assert same(h, c)
    # truncate_iteration keeps the FIRST rows of an iteration (Coach.loadTrainExamples drops from the end)
    h = DeviceHistory(S, A, P)
    for it in its[:2]:
        h.append_columns(it)
    h.truncate_iteration(0, 2)
    assert h.sizes == [2, 7] and same(h, cat([[x[:2] for x in its[0]], its[1]]))
    h.truncate_iteration(1, 7)
    assert h.sizes == [2, 7]


@pytest.mark.parametrize('compress', [True, False])
def test_round_trip_through_the_reference_layout(compress):
    from azg_amd import formats
    from azg_amd.history import DeviceHistory
    its = [make_cols(n, 10 + i) for i, n in enumerate((4, 0, 3))]
    h = DeviceHistory(S, A, P)
    for it in its:
        h.append_columns(it)
    ref = [h.to_reference(i, (3, 2), compress=compress, maxlen=50) for i in range(3)]
    assert [len(d) for d in ref] == [4, 0, 3] and all(d.maxlen == 50 for d in ref)
    e = ref[0][1] if not compress else pickle.loads(zlib.decompress(ref[0][1]))
    assert isinstance(ref[0][1], tuple) != compress
    assert e[0].shape == (3, 2) and e[0].dtype == np.int8 and e[3].dtype == bool and np.array_equal(e[1], its[0][1][1])
    # ... exactly what the default path builds from the same columns
    want = formats.examples_to_iteration(its[0], (3, 2), compress=compress, maxlen=50)
    assert all((a == b) if compress else all(np.array_equal(x, y) for x, y in zip(a, b)) for a, b in zip(ref[0], want))
    back = DeviceHistory.from_reference(ref)
    assert back.sizes == [4, 0, 3] and back.widths == (S, A, P, A, P) and same(back, cat(its))
    mixed = DeviceHistory.from_reference([list(ref[0]), ref[2]], widths=(S, A, P))            # lists and deques alike
    assert mixed.sizes == [4, 3] and same(mixed, cat([its[0], its[2]]))
    with pytest.raises(ValueError):
        DeviceHistory.from_reference([[], []])


def test_round_trip_through_the_column_file(tmp_path):
    from azg_amd.history import DeviceHistory
    its = [make_cols(n, 20 + i) for i, n in enumerate((5, 0, 2))]
    h = DeviceHistory(S, A, P, capacity=64)
    for it in its:
        h.append_columns(it)
    path = str(tmp_path / 'checkpoint.examples.npz')
    h.save_columns(path)
    assert os.path.exists(path) and os.listdir(tmp_path) == ['checkpoint.examples.npz']
    with np.load(path) as d:
        assert sorted(d.files) == ['boards', 'pi', 'q', 'sizes', 'valids', 'z'] and d['sizes'].tolist() == [5, 0, 2] and d['boards'].shape == (7, S)
    back = DeviceHistory.load_columns(path)
    assert back.sizes == [5, 0, 2] and same(back, cat(its))


def test_from_reference_reads_a_file_written_by_the_reference():
    """tests/golden/ref_checkpoint.examples: the reference's own Coach.saveTrainExamples, two iterations (4 + 2) of compressed Splendor-2p
    examples = the first six rows of the trainer fixture (tests/test_formats.py)"""
    import pickle
    from azg_amd.history import DeviceHistory
    with open(os.path.join(GOLDEN, 'ref_checkpoint.examples'), 'rb') as f:
        hist = pickle.load(f)
    h = DeviceHistory.from_reference(hist)
    d = np.load(os.path.join(GOLDEN, 'train_splendor2_v80.npz'))
    assert h.sizes == [4, 2] and h.widths == (392, 81, 2, 81, 2)
    want = [d['boards'][:6].reshape(6, -1), d['pi'][:6], d['z'][:6], d['valids'][:6].astype(np.uint8), d['q'][:6]]
    assert same(h, want)


def test_coach_signature_and_the_device_batches_requirement():
    from azg_amd.coach import Coach
    from azg_amd.history import DeviceHistory
    params = list(inspect.signature(Coach.__init__).parameters.values())
    assert [p.name for p in params][:8] == ['self', 'game', 'nnet', 'args', 'n_games', 'node_capacity', 'log', 'dist']
    assert params[-1].name == 'device_history' and params[-1].default is None
    assert [p.name for p in inspect.signature(DeviceHistory.append_records).parameters.values()] == ['self', 'game', 'records', 'maxlen', 'stream0']


# ---- code-object notes ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def notes():
    return kernel_notes(LIB)


@pytest.mark.skipif(not _BUILT, reason='needs the ROCm LLVM tools and the built library')
def test_there_is_one_examples_kernel_per_game_and_no_other(notes):
    ex = sorted(n.split('(')[0].replace('void azg::', '') for n in notes if 'k_examples_' in n)
    assert ex == sorted(VGPR_BOUNDS)


@pytest.mark.skipif(not _BUILT, reason='needs the ROCm LLVM tools and the built library')
@pytest.mark.parametrize('frag', sorted(VGPR_BOUNDS))
def test_examples_kernel_resources(notes, frag):
    """no scratch, no spilled register, LDS no larger than the k_env_symmetries* kernel of the same game, VGPRs within the bound"""
    k = [(n, v) for n, v in notes.items() if ('azg::' + frag + '(') in n]
    assert len(k) == 1, (frag, sorted(n for n in notes if 'k_examples_' in n))
    n, v = k[0]
    twin = [(m, w) for m, w in notes.items() if ('azg::' + frag.replace('k_examples_expand', 'k_env_symmetries') + '(') in m]
    assert len(twin) == 1, frag
    print(frag, v, 'symmetry kernel:', twin[0][1])
    assert v['lds'] <= twin[0][1]['lds'], (n, v, twin[0][1])
    assert v['vgpr'] <= VGPR_BOUNDS[frag], (n, v)
    assert v['vgpr_spill'] == 0 and v.get('sgpr_spill', 0) == 0, (n, v)
    assert v['scratch'] == 0, (n, v)
