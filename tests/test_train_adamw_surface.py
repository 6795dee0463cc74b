"""CPU: the surface of the device optimiser -- azg_train_adamw / azg_train_step_advance are declared in include/azg.h, exported by the built
library, bound and listed in _lib.EXPORTS; refused arguments return < 0 with the function's name before anything touches a GPU;
train.train's three new parameters default to the old behaviour and refuse a CPU device or a missing device_batches; the wrapper and
tools/train_offline.py pass the two switches on.

train.onecycle_adamw_table against torch itself: a real AdamW + OneCycleLR is stepped, lr and beta1 are read before each optimiser step, and
columns 0-5 must be the f32 casts of the formulas of torch's _multi_tensor_adamw on those values, bit for bit.

The restatement and its bound (adamw_f64 / adamw_bounds, shared with tests/test_gpu_train_adamw.py): one AdamW step evaluated in float64 with
float64 scalars, and for an f32 evaluation with one rounding per operation and one per scalar cast, u = 2^-24, all quantities from the
float64 evaluation (v' the new second moment, D = step_size m' / denom the parameter's move):
    |dm| <= 4u (|m| + |g|)          g - m, its product with 1 - beta1 (a cast scalar) and the sum: 4 roundings of terms each bounded by |m| + |g|
    |dv| <= 6u v'                   v beta2 (2: cast, product), g g (1 - beta2) (3), the sum (1): every term is positive and at most v'
    |dp| <= 3u (|p| + |D|) + (step_size / denom) 4u (|m| + |g|) + 12u |D|
                                    p (1 - lr wd) and the difference (3); the error of m' carried through the quotient; and D's own chain:
                                    sqrt(v') with v' 6u off (3u) + its rounding, / sqrt(bias2) (2), + eps (2), m' / d (1), step_size (2): 11, within 12
torch's own CPU AdamW (foreach=False) must meet them: a bound the reference does not meet would be no bound for the kernel.  Measured: torch
uses at most 0.72 of |dp|, 0.19 of |dm| and 0.40 of |dv| over the six cases below."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('azg_train_adamw', 'azg_train_step_advance')
U = 2.0 ** -24


def adamw_f64(p, g, m, v, lr, beta1, beta2, eps, wd, k):
    """one AdamW step (optimiser step number k, 1-based) in float64 from f32 inputs, the scalars as Python floats
    -> p', m', v', D = step_size m' / denom, step_size / denom"""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    m2 = m + (1.0 - beta1) * (g - m)
    v2 = v * beta2 + (1.0 - beta2) * g * g
    denom = np.sqrt(v2) / math.sqrt(1.0 - beta2 ** k) + eps
    step_size = lr / (1.0 - beta1 ** k)
    delta = step_size * m2 / denom
    return p * (1.0 - lr * wd) - delta, m2, v2, delta, step_size / denom


def adamw_bounds(p, g, m, v2, delta, ss_over_denom):
    """-> the bounds on |dp|, |dm|, |dv| of the module docstring"""
    p, g, m = (np.abs(np.asarray(x, dtype=np.float64)) for x in (p, g, m))
    bm = 4 * U * (m + g)
    return 3 * U * (p + np.abs(delta)) + ss_over_denom * bm + 12 * U * np.abs(delta), bm, 6 * U * v2


def torch_schedule(total_steps, max_lr):
    """[(lr, beta1)] that a real AdamW + OneCycleLR holds before each of its total_steps optimiser steps"""
    import torch
    w = torch.nn.Parameter(torch.zeros(1))
    w.grad = torch.zeros(1)
    opt = torch.optim.AdamW([w], lr=max_lr)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=max_lr, total_steps=total_steps)
    out = []
    for _ in range(total_steps):
        out.append((opt.param_groups[0]['lr'], opt.param_groups[0]['betas'][0]))
        opt.step()
        sched.step()
    return out


def test_entry_points_are_declared_exported_and_bound():
    from azg_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'azg.h')).read()
    L = _lib.lib()
    for name in NAMES:
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None, name
    assert len(L.azg_train_adamw.argtypes) == 8 and len(L.azg_train_step_advance.argtypes) == 2
    # the three entry points of the batch side keep their signatures
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

    def adamw(n_segs=2, n_chunks=3, total=10, **null):
        a = {k: (None if k in null else p) for k in ('segs', 'chunks', 'table', 'step')}
        return L.azg_train_adamw(a['segs'], n_segs, a['chunks'], n_chunks, a['table'], total, a['step'], None)

    for kw in (dict(segs=None), dict(chunks=None), dict(table=None), dict(step=None), dict(n_segs=0), dict(n_segs=-1), dict(n_chunks=0),
               dict(n_chunks=-5), dict(total=0), dict(total=-1)):
        refused(adamw(**kw), 'azg_train_adamw')
    refused(L.azg_train_step_advance(None, None), 'azg_train_step_advance')


def _tiny_examples():
    return (np.zeros((4, 392), np.int8), np.full((4, 81), 1 / 81, np.float32), np.zeros((4, 2), np.float32), np.ones((4, 81), np.uint8),
            np.zeros((4, 2), np.float32))


def test_train_defaults_and_the_refusals():
    from azg_amd import train
    sig = inspect.signature(train.train)
    assert sig.parameters['device_optimizer'].default is False and sig.parameters['graph_step'].default is False
    assert sig.parameters['info'].default is None
    assert sig.parameters['device_batches'].default is False                       # (and the earlier switch stays off)
    for name in ('onecycle_adamw_table', 'DeviceAdamW', 'adamw_tables', 'adamw_update', 'adamw_step_advance'):
        assert callable(getattr(train, name))
    ex = _tiny_examples()
    with pytest.raises(ValueError, match='device_optimizer'):
        train.train(train.SplendorV80Module(), ex, batch_size=2, epochs=1, device='cpu', device_batches=True, device_optimizer=True)
    with pytest.raises(ValueError, match='device_optimizer'):
        train.train(train.SplendorV80Module(), ex, batch_size=2, epochs=1, device='cuda:0', device_optimizer=True)
    with pytest.raises(ValueError, match='graph_step'):
        train.train(train.SplendorV80Module(), ex, batch_size=2, epochs=1, device='cpu', device_batches=True, graph_step=True)
    with pytest.raises(ValueError, match='device_optimizer'):
        train.train(train.SplendorV80Module(), ex, batch_size=2, epochs=1, device='cuda:0', graph_step=True)


def test_info_names_the_optimizer_on_the_default_path():
    import torch
    from azg_amd import train
    torch.manual_seed(0)
    info = {}
    hist = train.train(train.SplendorV80Module(), _tiny_examples(), batch_size=2, epochs=1, device='cpu', seed=1, info=info)
    assert len(hist) == 2 and info == {'optimizer': 'torch', 'graph_replays': 0}


def test_nnet_wrapper_passes_both_switches_on(monkeypatch):
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
    cols = [np.zeros((8, 1), np.float32) for _ in range(5)]                          # five arrays pass through _cols
    w.args = dict(batch_size=8)
    w.train(cols)
    assert seen['device_optimizer'] is False and seen['graph_step'] is False and seen['device_batches'] is False
    w.args = dict(batch_size=8, device_batches=True, device_optimizer=True)
    w.train(cols)
    assert seen['device_optimizer'] is True and seen['graph_step'] is False and seen['device_batches'] is True
    w.args = dict(batch_size=8, device_batches=True, graph_step=True)
    w.train(cols)
    assert seen['graph_step'] is True


def test_train_offline_lists_both_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train_offline.py'), '--help'], capture_output=True, text=True, check=True).stdout
    assert '--device-optimizer' in out and '--graph-step' in out


@pytest.mark.parametrize('total_steps,max_lr', [(1, 3e-3), (2, 3e-3), (10, 3e-3), (257, 1e-2)])
def test_table_equals_torchs_own_schedule_bit_for_bit(total_steps, max_lr):
    from azg_amd import train
    table = np.asarray(train.onecycle_adamw_table(max_lr, total_steps))
    assert table.dtype == np.float32 and table.shape == (total_steps, 8)
    beta2, eps, wd = 0.999, 1e-8, 1e-2
    sched = torch_schedule(total_steps, max_lr)
    for s, (lr, beta1) in enumerate(sched):
        k = s + 1
        want = np.array([1 - lr * wd, 1 - beta1, beta2, 1 - beta2, lr / (1 - beta1 ** k), math.sqrt(1 - beta2 ** k)]).astype(np.float32)
        assert np.array_equal(table[s, :6].view(np.uint32), want.view(np.uint32)), (s, table[s], want)
        assert table[s, 6] == np.float32(eps) and table[s, 7] == 0
    if (total_steps, max_lr) == (10, 3e-3):                                          # the schedule itself: warm-up, peak, anneal; momentum inverse
        lrs, b1 = [x[0] for x in sched], [x[1] for x in sched]
        assert abs(lrs[0] - 1.2e-4) < 1e-12 and abs(lrs[2] - 3e-3) < 1e-12 and abs(lrs[-1] - 1.2e-8) < 1e-14
        assert abs(b1[0] - 0.95) < 1e-12 and abs(b1[2] - 0.85) < 1e-12 and abs(b1[-1] - 0.95) < 1e-12


def test_table_with_other_betas_eps_and_decay():
    from azg_amd import train
    t = np.asarray(train.onecycle_adamw_table(1e-3, 4, betas=(0.9, 0.99), eps=1e-6, weight_decay=0.1))
    assert np.array_equal(t[:, 2], np.full(4, np.float32(0.99))) and np.array_equal(t[:, 6], np.full(4, np.float32(1e-6)))
    lr0 = 1e-3 / 25
    assert t[0, 0] == np.float32(1 - lr0 * 0.1) and t[0, 1] == np.float32(1 - 0.95)  # OneCycleLR cycles beta1 whatever betas[0] says
    with pytest.raises(ValueError, match='total_steps'):
        train.onecycle_adamw_table(1e-3, 0)


@pytest.mark.parametrize('k', [1, 2, 1000])
@pytest.mark.parametrize('g_scale', [1.0, 1e-4])
def test_torchs_cpu_adamw_meets_the_bounds_of_the_restatement(k, g_scale):
    import torch
    lr, beta1, beta2, eps, wd = 3e-3, 0.9, 0.999, 1e-8, 1e-2
    r = np.random.RandomState(1000 * k + int(g_scale * 10))
    n = 4096
    p = r.randn(n).astype(np.float32)
    g = (r.randn(n) * g_scale).astype(np.float32)
    m = (r.randn(n) * 0.1 * g_scale).astype(np.float32)
    v = ((r.randn(n) * 0.1 * g_scale) ** 2).astype(np.float32)
    w = torch.nn.Parameter(torch.from_numpy(p.copy()))
    w.grad = torch.from_numpy(g.copy())
    opt = torch.optim.AdamW([w], lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[w] = dict(step=torch.tensor(float(k - 1)), exp_avg=torch.from_numpy(m.copy()), exp_avg_sq=torch.from_numpy(v.copy()))
    opt.step()
    assert float(opt.state[w]['step']) == k
    p2, m2, v2, delta, ssd = adamw_f64(p, g, m, v, lr, beta1, beta2, eps, wd, k)
    bp, bm, bv = adamw_bounds(p, g, m, v2, delta, ssd)
    ep = np.abs(w.detach().numpy().astype(np.float64) - p2)
    em = np.abs(opt.state[w]['exp_avg'].numpy().astype(np.float64) - m2)
    ev = np.abs(opt.state[w]['exp_avg_sq'].numpy().astype(np.float64) - v2)
    print('torch CPU AdamW, k = %d, gradient scale %g: largest share of the bounds used: p %.2f, m %.2f, v %.2f'
          % (k, g_scale, (ep / bp).max(), (em / bm).max(), (ev / bv).max()))
    assert (ep <= bp).all() and (em <= bm).all() and (ev <= bv).all()
    assert ep.max() > 0                                                              # (the comparison is not one of a thing with itself)
