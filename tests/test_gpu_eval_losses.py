"""GPU: azg_eval_losses (csrc/loss.hip.h; nnet.eval_losses) against a NumPy float64 restatement of train.loss_pi / train.loss_v, written
here from the formulas of include/azg.h -- the kernel is never compared with itself:
  rows[b, 0]  = sum over the actions with t > 0 of t (log t - log max(pi, FLT_MIN))       (an action with t == 0 adds exactly 0)
  rows[b, 1]  = sum_p ((z + q_weight q) / (1 + q_weight) - v)^2                            (q_weight as the f32 the C-ABI takes)
  flags[b, 0] = np.argmax(t) == np.argmax(pi)   (first index on ties),   flags[b, 1] = #(t > 0 and pi < FLT_MIN)

The bound is derived, not measured.  Both sides compute every term from the same f32 inputs in f64; a term t (log t - log p) carries the
error of two logs (about an ulp of |log t| and of |log p| each), one subtraction and one product, and a sum of A terms in another order
differs by at most (A - 1) ulp of the sum of their magnitudes.  Hence per entry of rows
    |kernel - restatement| <= (A + 8) 2^-52 sum |terms of that row|,   |term| counted as t (|log t| + |log p|)  resp.  d^2,
with the sum of magnitudes taken from the restatement.  The squared errors use IEEE operations only (no contraction: the library is built
with -ffp-contract=off), so only the order of their <= 8 terms differs.  flags are exact.  totals sum B rows: B 2^-52 sum |rows|.

Shapes: A = 21 (a row shorter than a wave), 81 (not a multiple of 64), 3402 (54 words per lane, not a multiple of 64); P = 2, 5;
B = 1, 3, 65 (one more row than a wave of the totals pass holds)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLT_MIN = np.float32(1.17549435e-38)
SHAPES = [(A, P, B) for A in (21, 81, 3402) for P in (2, 5) for B in (1, 3, 65)]
Q_WEIGHT = 0.3                      # (not a binary fraction: the restatement must round it to f32 as the C-ABI does)


def make_inputs(A, P, B, seed=0, support_only=True):
    """-> dict of f32 arrays.  Targets: random on a random set of 'valid' actions, normalised, EXACT zeros elsewhere.  pi: a softmax over the
    valid actions, 0 on the others (support_only: what an engine net returns), then per row
      b % 3 == 0: pi = 0 on one action with t > 0                        -> floored there, counted in flags[:, 1]
      b % 3 == 1 (and the single row of B == 1): the maximum of pi twice, the target's maximum on the first or the second of the two
      b % 3 == 2: a subnormal pi (1e-40 < FLT_MIN) on one action with t > 0 -> floored too"""
    r = np.random.RandomState(seed + 7 * A + 100 * P + B)
    valid = r.rand(B, A) < 0.5
    valid[:, :4] = True
    t = np.where(valid, r.rand(B, A) + 0.01, 0.0)
    t = (t / t.sum(1, keepdims=True)).astype(np.float32)
    logits = r.randn(B, A) * 2.0
    e = np.where(valid, np.exp(logits), 0.0 if support_only else 1e-6)
    pi = (e / e.sum(1, keepdims=True)).astype(np.float32)
    for b in range(B):
        sup = np.flatnonzero(valid[b])
        if b % 3 == 0:
            pi[b, sup[1]] = 0.0
        if b % 3 == 1 or B == 1:
            i, j = sup[2], sup[-1]                                    # i < j, both on the support
            pi[b, i] = pi[b, j] = np.float32(pi[b].max() * 1.5)
            t[b, j if b % 2 == 0 and B > 1 else i] = np.float32(t[b].max() * 1.25)   # (rows stay near-normalised: the kernel does not care)
        if b % 3 == 2:
            pi[b, sup[3]] = np.float32(1e-40)
    assert (t[~valid] == 0).all() and (not support_only or (pi[~valid] == 0).all())
    v = np.tanh(r.randn(B, P)).astype(np.float32)
    z = r.uniform(-1, 1, (B, P)).astype(np.float32)
    q = r.uniform(-1, 1, (B, P)).astype(np.float32)
    return dict(pi=pi, v=v, target_pi=t, z=z, q=q)


def restate(d, q_weight, active=None):
    """-> rows f64[B, 2], the sums of the terms' magnitudes f64[B, 2], flags i64[B, 2]"""
    t, pi = d['target_pi'].astype(np.float64), d['pi']
    pos = d['target_pi'] > 0
    p = np.maximum(pi, FLT_MIN).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        lt, lp = np.where(pos, np.log(np.where(pos, t, 1.0)), 0.0), np.where(pos, np.log(p), 0.0)
    kl, kl_abs = np.where(pos, t * (lt - lp), 0.0), np.where(pos, t * (np.abs(lt) + np.abs(lp)), 0.0)
    qw = np.float64(np.float32(q_weight))
    dv = (d['z'].astype(np.float64) + qw * d['q'].astype(np.float64)) / (1.0 + qw) - d['v'].astype(np.float64)
    rows = np.stack([kl.sum(1), (dv * dv).sum(1)], axis=1)
    mags = np.stack([kl_abs.sum(1), (dv * dv).sum(1)], axis=1)
    flags = np.stack([(np.argmax(d['target_pi'], 1) == np.argmax(pi, 1)).astype(np.int64), (pos & (pi < FLT_MIN)).sum(1)], axis=1)
    if active is not None:
        keep = np.asarray(active).astype(bool)[:, None]
        rows, mags, flags = rows * keep, mags * keep, flags * keep
    return rows, mags, flags


def run(d, q_weight, active=None, totals=None, accumulate=False):
    import torch
    from azg_amd import nnet
    dev = {k: torch.from_numpy(np.ascontiguousarray(x)).cuda() for k, x in d.items()}
    act = None if active is None else torch.from_numpy(np.asarray(active, dtype=np.uint8)).cuda()
    rows, flags, totals = nnet.eval_losses(dev['pi'], dev['v'], dev['target_pi'], dev['z'], dev['q'], q_weight, active=act, totals=totals,
                                           accumulate=accumulate)
    return rows.cpu().numpy(), flags.cpu().numpy(), totals


def check_rows(rows, flags, d, q_weight, A, active=None):
    want, mags, wflags = restate(d, q_weight, active)
    bound = (A + 8) * 2.0 ** -52 * mags
    err = np.abs(rows - want)
    print('max |kernel - restatement| / bound: KL %.3g, SE %.3g' % tuple((err / np.maximum(bound, 1e-300)).max(0)))
    assert np.isfinite(rows).all()
    assert (err <= bound).all(), (err.max(0), bound.min(0))
    assert np.array_equal(flags.astype(np.int64), wflags)
    return want, mags, wflags


@pytest.mark.parametrize('A,P,B', SHAPES)
def test_rows_flags_and_totals_against_the_restatement(A, P, B):
    d = make_inputs(A, P, B)
    rows, flags, totals = run(d, Q_WEIGHT)
    want, mags, wflags = check_rows(rows, flags, d, Q_WEIGHT, A)
    # the inputs hold what they are meant to hold
    assert wflags[0, 1] == 1 and (B < 3 or wflags[2, 1] == 1)                          # pi == 0 / subnormal where t > 0: floored, finite
    if B > 1:
        assert wflags[1, 0] == 1 and (B < 5 or wflags[4, 0] == 0)                      # the tie: the first index wins
    tot = totals.cpu().numpy()
    tb = B * 2.0 ** -52 * np.abs(rows).sum(0)
    assert (np.abs(tot[:2] - rows.sum(0)) <= tb).all(), (tot, rows.sum(0), tb)
    assert tot[2] == flags[:, 0].sum() and tot[3] == flags[:, 1].sum()


@pytest.mark.parametrize('A,P,B', [(81, 2, 65), (3402, 5, 3)])
def test_zero_target_adds_exactly_nothing(A, P, B):
    """t == 0 contributes exactly 0 whatever pi is there: 0, a probability, inf or NaN"""
    d = make_inputs(A, P, B)
    rows0, flags0, _ = run(d, Q_WEIGHT)
    off = d['target_pi'] == 0
    for fill in (0.25, np.inf, np.nan, 0.0):
        e = dict(d, pi=np.where(off, np.float32(fill), d['pi']).astype(np.float32))
        rows, flags, _ = run(e, Q_WEIGHT)
        assert np.array_equal(rows, rows0) and np.array_equal(flags[:, 1], flags0[:, 1]), fill


def test_inactive_rows_write_zeros_and_count_for_nothing():
    A, P, B = 81, 5, 65
    d = make_inputs(A, P, B)
    active = (np.arange(B) % 4 != 1).astype(np.uint8)
    rows, flags, totals = run(d, Q_WEIGHT, active=active)
    check_rows(rows, flags, d, Q_WEIGHT, A, active)
    assert (rows[active == 0] == 0).all() and (flags[active == 0] == 0).all()
    full_rows, full_flags, _ = run(d, Q_WEIGHT)
    assert np.array_equal(rows[active == 1], full_rows[active == 1]) and np.array_equal(flags[active == 1], full_flags[active == 1])
    tot, on = totals.cpu().numpy(), active == 1
    assert (np.abs(tot[:2] - full_rows[on].sum(0)) <= B * 2.0 ** -52 * np.abs(full_rows[on]).sum(0)).all()
    assert tot[2] == full_flags[on, 0].sum() and tot[3] == full_flags[on, 1].sum()


@pytest.mark.parametrize('A,P,B', [(21, 2, 65), (3402, 2, 3), (81, 5, 1)])
def test_accumulate_over_two_chunks_equals_one_call(A, P, B):
    d = make_inputs(A, P, B)
    rows, _, one = run(d, Q_WEIGHT)
    h = B // 2                                                                     # (B == 1: an empty first chunk)
    _, _, tot = run({k: x[:h] for k, x in d.items()}, Q_WEIGHT)
    _, _, tot = run({k: x[h:] for k, x in d.items()}, Q_WEIGHT, totals=tot, accumulate=True)
    one, two = one.cpu().numpy(), tot.cpu().numpy()
    assert (np.abs(one[:2] - two[:2]) <= B * 2.0 ** -52 * np.abs(rows).sum(0)).all(), (one, two)
    assert np.array_equal(one[2:], two[2:])


def test_two_calls_are_bit_identical_and_a_row_does_not_depend_on_B():
    A, P, B = 3402, 5, 65
    d = make_inputs(A, P, B)
    r1, f1, t1 = run(d, Q_WEIGHT)
    r2, f2, t2 = run(d, Q_WEIGHT)
    assert np.array_equal(r1, r2) and np.array_equal(f1, f2) and np.array_equal(t1.cpu().numpy(), t2.cpu().numpy())
    for b in (0, 31, 64):
        rb, fb, _ = run({k: x[b:b + 1] for k, x in d.items()}, Q_WEIGHT)
        assert np.array_equal(rb[0], r1[b]) and np.array_equal(fb[0], f1[b])


def test_no_rows():
    import torch
    d = {k: x[:0] for k, x in make_inputs(21, 2, 1).items()}
    rows, flags, totals = run(d, Q_WEIGHT)
    assert rows.shape == (0, 2) and flags.shape == (0, 2) and (totals.cpu().numpy() == 0).all()
    keep = torch.tensor([1.5, 2.5, 3.0, 4.0], dtype=torch.float64, device='cuda:0')
    _, _, totals = run(d, Q_WEIGHT, totals=keep, accumulate=True)
    assert totals.cpu().tolist() == [1.5, 2.5, 3.0, 4.0]
    _, _, totals = run(d, Q_WEIGHT, totals=keep)                                   # without accumulate: zeroed
    assert totals.cpu().tolist() == [0.0] * 4


def test_refused_arguments_return_a_text_and_launch_nothing():
    import torch
    from azg_amd import _lib
    A, P, B = 21, 2, 3
    d = {k: torch.from_numpy(x).cuda() for k, x in make_inputs(A, P, B).items()}
    rows = torch.full((B, 2), -7.0, dtype=torch.float64, device='cuda:0')
    flags = torch.full((B, 2), -7, dtype=torch.int32, device='cuda:0')
    totals = torch.full((4,), -7.0, dtype=torch.float64, device='cuda:0')
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731

    def call(B=B, A=A, P=P, qw=0.5, **over):
        a = dict(d, rows=rows, flags=flags, totals=totals)
        a.update(over)
        return _lib.lib().azg_eval_losses(ptr(a['pi']), ptr(a['v']), ptr(a['target_pi']), ptr(a['z']), ptr(a['q']), None, B, A, P, C.c_float(qw),
                                          ptr(a['rows']), ptr(a['flags']), ptr(a['totals']), 0, None)

    bad = [dict(B=-1), dict(A=0), dict(P=0), dict(P=9), dict(qw=-1.0), dict(qw=-2.0)] + \
          [{k: None} for k in ('pi', 'v', 'target_pi', 'z', 'q', 'rows', 'flags', 'totals')]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert 'azg_eval_losses' in _lib.lib().azg_last_error().decode(), kw
    torch.cuda.synchronize()
    assert (rows == -7).all() and (flags == -7).all() and (totals == -7).all()
    assert call() == 0                                                             # the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert (rows != -7).all() and (totals != -7).all()


@pytest.mark.parametrize('A,P,B', [(21, 5, 65), (81, 2, 65), (3402, 5, 65)])
def test_totals_against_torch_float64(A, P, B):
    """F.kl_div(log pi, t, 'batchmean') and train.loss_v in float64 on the same tensors: 1e-12 relative.  pi is strictly positive here
    (torch has nothing to floor, and 0 * log 0 off the support would be a NaN there), the targets keep their exact zeros; q_weight = 0.5
    is the same number in f32 and f64."""
    import torch
    import torch.nn.functional as F
    from azg_amd import train
    d = make_inputs(A, P, B, seed=5, support_only=False)
    d['pi'] = np.maximum(d['pi'], np.float32(1e-30))                               # (the zero / subnormal entries of make_inputs)
    _, flags, totals = run(d, 0.5)
    assert flags[:, 1].sum() == 0
    t64 = {k: torch.from_numpy(x).cuda().double() for k, x in d.items()}
    l_pi = F.kl_div(torch.log(t64['pi']), t64['target_pi'], reduction='batchmean').item()
    l_v = train.loss_v(t64['z'], t64['q'], t64['v'], 0.5).item()
    tot = totals.cpu().numpy()
    print('loss_pi %.17g vs %.17g   loss_v %.17g vs %.17g' % (tot[0] / B, l_pi, tot[1] / (B * P), l_v))
    assert abs(tot[0] / B - l_pi) <= 1e-12 * abs(l_pi) and abs(tot[1] / (B * P) - l_v) <= 1e-12 * abs(l_v)
