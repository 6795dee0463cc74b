"""CPU: the surface of the device-batch training path -- azg_train_sample_ids / azg_train_gather / azg_train_losses are declared in
include/azg.h, exported by the built library, bound and listed in _lib.EXPORTS; refused arguments return < 0 with a message before anything
touches a GPU; train.train's new parameters default to the old behaviour and refuse a CPU device; tools/train_offline.py has the flag.

Code-object notes of the four new kernels, read as tests/test_eval_losses_resources.py reads them: no scratch, no spilled register; the
gather and loss kernels use no LDS; the sampler's map (2 x 64 KiB of keys and values + 64 staged indices) stays within a CU's 160 KiB.
Measured build: k_train_sample_ids 9 VGPRs, k_train_gather 59, k_train_loss_rows 42, k_train_loss_totals 30 -- each bounded at the next
multiple of 16 above (16 / 64 / 48 / 32)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import pytest

from test_kernel_resources import LIB, LLVM, kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('azg_train_sample_ids', 'azg_train_gather', 'azg_train_losses')
_BUILT = os.path.exists(os.path.join(LLVM, 'llvm-readelf')) and os.path.exists(LIB)


def test_entry_points_are_declared_exported_and_bound():
    from azg_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'azg.h')).read()
    L = _lib.lib()
    for name in NAMES:
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in _lib.EXPORTS
        fn = getattr(L, name)                                                       # exported by the library
        assert fn.argtypes is not None and len(fn.argtypes) >= 7, name              # bound
    assert len(L.azg_train_sample_ids.argtypes) == 7 and len(L.azg_train_gather.argtypes) == 17 and len(L.azg_train_losses.argtypes) == 15


def test_refused_arguments_return_a_text_before_any_launch():
    """every call below is refused by the argument checks, which run before the first HIP call: no GPU is needed (the pointers are fakes
    that are never followed)"""
    from azg_amd import _lib
    L = _lib.lib()
    p = C.c_void_p(0x1000)

    def refused(rc, name):
        assert rc < 0, name
        msg = L.azg_last_error().decode()
        assert name in msg and len(msg) > len(name) + 4, msg

    for n, batch, steps, ids in ((4, 5, 1, p), (100000, 8193, 1, p), (2 ** 31, 4, 1, p), (10, 0, 1, p), (10, 4, -1, p), (10, 4, 1, None)):
        refused(L.azg_train_sample_ids(n, batch, steps, 0, 0, ids, None), 'azg_train_sample_ids')

    def gather(n=10, B=4, S=75, A=21, P=5, **null):
        a = [None if k in null else p for k in ('boards', 'pi', 'z', 'valids', 'q', 'ids')]
        o = [None if k in null else p for k in ('out_boards', 'out_pi', 'out_z', 'out_valids', 'out_q')]
        return L.azg_train_gather(*a, n, B, S, A, P, *o, None)

    for kw in (dict(P=9), dict(P=0), dict(B=-1), dict(S=0), dict(A=0), dict(n=0), dict(ids=None), dict(boards=None), dict(out_valids=None)):
        refused(gather(**kw), 'azg_train_gather')

    def losses(B=4, A=21, P=2, qw=0.5, **null):
        a = [None if k in null else p for k in ('log_pi', 'v', 'target_pi', 'z', 'q')]
        o = [None if k in null else p for k in ('grad_log_pi', 'grad_v', 'rows', 'out')]
        return L.azg_train_losses(*a, B, A, P, C.c_float(qw), C.c_float(0.25), *o, None)

    for kw in (dict(P=9), dict(P=0), dict(B=0), dict(A=0), dict(qw=-1.0), dict(qw=-2.0), dict(qw=float('nan')), dict(log_pi=None), dict(rows=None),
               dict(out=None), dict(grad_v=None)):
        refused(losses(**kw), 'azg_train_losses')


def test_train_defaults_and_the_cpu_refusal():
    import numpy as np
    from azg_amd import train
    sig = inspect.signature(train.train)
    assert sig.parameters['device_batches'].default is False and sig.parameters['batch_ids'].default is None
    for name in ('sample_ids', 'gather_batch', 'train_losses', 'fused_loss'):
        assert callable(getattr(train, name))
    assert inspect.signature(train.fused_loss).parameters['v_coeff'].default == 0.25
    ex = (np.zeros((4, 392), np.int8), np.full((4, 81), 1 / 81, np.float32), np.zeros((4, 2), np.float32), np.ones((4, 81), np.uint8),
          np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError, match='device_batches'):
        train.train(train.SplendorV80Module(), ex, batch_size=2, epochs=1, device='cpu', device_batches=True)


def test_batch_ids_replace_the_draw_on_the_cpu_path():
    """batch_ids feed the legacy path too: the same rows give the same history whatever the seed, and a wrong shape is refused"""
    import numpy as np
    import torch
    from azg_amd import train
    rng = np.random.default_rng(0)
    n = 16
    pi = rng.random((n, 81)).astype(np.float32)
    ex = (rng.integers(0, 5, (n, 392)).astype(np.int8), pi / pi.sum(1, keepdims=True), rng.uniform(-1, 1, (n, 2)).astype(np.float32),
          np.ones((n, 81), np.uint8), rng.uniform(-1, 1, (n, 2)).astype(np.float32))
    ids = np.stack([rng.permutation(n)[:4] for _ in range(4)])

    def run(seed, batch_ids):
        torch.manual_seed(0)
        return train.train(train.SplendorV80Module(), ex, batch_size=4, epochs=1, device='cpu', seed=seed, batch_ids=batch_ids)

    assert run(1, ids) == run(2, ids)
    assert run(1, None) != run(1, ids)
    with pytest.raises(ValueError, match='batch_ids'):
        run(1, ids[:3])


def test_nnet_wrapper_passes_device_batches_on(monkeypatch):
    from azg_amd import nnet_wrapper
    seen = {}

    def fake_train(module, cols, **kw):
        seen.update(kw)
        return []

    monkeypatch.setattr(nnet_wrapper._train, 'train', fake_train)
    w = nnet_wrapper.NNetWrapper.__new__(nnet_wrapper.NNetWrapper)

    class G:
        device = 'cpu'

    w.game, w.nnet, w._custom, w.board_size, w._eval = G(), None, False, (56, 7), None
    import numpy as np
    cols = [np.zeros((8, 1), np.float32) for _ in range(5)]                          # five arrays pass through _cols
    w.args = dict(batch_size=8)
    w.train(cols)
    assert seen['device_batches'] is False
    w.args = dict(batch_size=8, device_batches=True)
    w.train(cols)
    assert seen['device_batches'] is True


def test_train_offline_lists_the_flag():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train_offline.py'), '--help'], capture_output=True, text=True, check=True).stdout
    assert '--device-batches' in out


@pytest.mark.skipif(not _BUILT, reason='needs the ROCm LLVM tools and the built library')
def test_new_kernels_need_no_scratch_and_stay_within_their_registers_and_lds():
    notes = kernel_notes(LIB)
    bounds = {'k_train_sample_ids(': 16, 'k_train_gather(': 64, 'k_train_loss_rows(': 48, 'k_train_loss_totals(': 32}
    for frag, vgpr_max in bounds.items():
        k = [(n, v) for n, v in notes.items() if frag in n]
        assert len(k) == 1, (frag, sorted(n for n in notes if 'k_train' in n))
        n, v = k[0]
        assert v['scratch'] == 0 and v['vgpr_spill'] == 0 and v.get('sgpr_spill', 0) == 0, (n, v)
        assert v['vgpr'] <= vgpr_max, (n, v)
        if 'sample_ids' in frag:
            assert 0 < v['lds'] <= 160 * 1024, (n, v)
        else:
            assert v['lds'] == 0, (n, v)
    assert len([n for n in notes if 'k_train_' in n]) == 4
