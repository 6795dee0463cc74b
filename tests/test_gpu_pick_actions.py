"""GPU: azg_pick_actions (csrc/pick.hip.h; arena.pick_actions) against a NumPy restatement of its three modes.

The uniform u of a draw is never re-derived here: it comes from the engine's own device generator through the test aid
azg_debug_rng_u01(seed, stream, counter).  The restatement then says what the kernel must do with it:
  mode 0  the floor(u nv)-th of the nv valid actions in index order (clamped to nv - 1)
  mode 1  the first index of the maximum over the valid, non-NaN entries; none -> 0
  mode 2  weights = probs where valid and > 0 (a NaN weighs nothing); the first index whose f64 cumulative sum exceeds u * total; none
          (rounding, or a total of 0) -> the last valid index
A row WITHOUT a valid action gives action 0 in every mode, and in modes 0 and 2 its counter still advances by one: the draw is taken
before the row is looked at, so that the number of draws of a game never depends on its masks.  Mode 1 draws nothing.

The kernel sums a row lane-strided and chunk by chunk, NumPy sequentially.  The probabilities of the exact-equality cases are multiples
of 2^-16 below 1: every partial sum of up to 3402 of them is exact in f64 in any order, so both sides compare the same numbers with
u * total.  test_sample_general_floats covers arbitrary f32 rows with the bound that the two summation orders allow.

Shapes: A = 21 (one chunk, lanes 21..63 idle), 81 (crosses the 63 / 64 lane stride), 3402 (54 chunks, not a multiple of 64); T = 1, 3, 65."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, STREAM0 = 0x5EED, (3 << 30) + 11
N_SEARCH = 4096                     # counters searched for a u near 1: the largest of 4096 uniforms is below 0.99 with probability 0.99^4096 < 1e-17


def draws(stream0, counter0, n_streams, n_counters, seed=SEED):
    """u01(seed, stream0 + i, counter0 + j) as f64[n_streams, n_counters], from the engine's device generator"""
    import torch
    from azg_amd import _lib
    out = torch.empty((n_streams, n_counters), dtype=torch.float64, device='cuda:0')
    _lib.check(_lib.lib().azg_debug_rng_u01(seed, stream0, counter0, n_streams, n_counters, C.c_void_p(out.data_ptr()),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out.cpu().numpy()


def ref_pick(mode, probs, valid, u):
    v = valid.astype(bool)
    idx = np.flatnonzero(v)
    if mode == 0:
        return int(idx[min(int(np.floor(u * len(idx))), len(idx) - 1)]) if len(idx) else 0
    if mode == 1:
        cand = np.flatnonzero(v & ~np.isnan(probs))
        return int(cand[np.argmax(probs[cand])]) if len(cand) else 0
    if not len(idx):
        return 0
    with np.errstate(invalid='ignore'):
        w = np.where(v & (probs > 0), probs, np.float32(0)).astype(np.float64)
    cum = np.cumsum(w)
    hit = np.flatnonzero(cum > u * cum[-1])
    return int(hit[0]) if len(hit) else int(idx[-1])


def row_patterns(A):
    """[(name, probs f32[A], valid u8[A])]: the rows every A is tested with.  Indices 63, 64 and 70 exist only where A allows them; the
    second maximum of the tie then sits at A - 1."""
    r = np.random.RandomState(1000 + A)
    base = (r.randint(1, 1 << 16, size=A) / 65536.0).astype(np.float32)
    ones, rows = np.ones(A, np.uint8), []
    for k in sorted({0, 63, 64, A - 1}):
        if k < A:
            v = np.zeros(A, np.uint8)
            v[k] = 1
            rows.append(('one_valid_%d' % k, base, v))
    rows.append(('all_valid', base, ones))
    rows.append(('none_valid', base, np.zeros(A, np.uint8)))
    tie2 = 70 if A > 70 else A - 1
    p = (base * np.float32(0.5)).astype(np.float32)
    p[5] = p[tie2] = 0.75
    rows.append(('tie_5_%d' % tie2, p, ones))
    v = ones.copy()
    v[5] = 0
    rows.append(('tie_first_masked', p, v))
    p = base.copy()
    p[0] = np.nan
    rows.append(('nan_at_0', p, ones))
    rows.append(('all_nan', np.full(A, np.nan, np.float32), ones))
    v = (r.rand(A) < 0.3).astype(np.uint8)
    v[A // 2] = 1
    p = np.zeros(A, np.float32)
    p[np.flatnonzero(v)[-1]] = 1.0
    rows.append(('mass_on_last_valid', p, v))
    rows.append(('u_near_1', base, ones))
    v = (r.rand(A) < 0.3).astype(np.uint8)
    v[A - 1] = 0
    rows.append(('sparse', base, v))
    return rows


def run(mode, probs, valid, counters, active=None, sentinel=0, stream0=STREAM0):
    import torch
    from azg_amd.arena import pick_actions
    dev = 'cuda:0'
    T = len(counters)
    cnt = torch.from_numpy(np.asarray(counters, dtype=np.int64)).to(dev)
    out = torch.full((T,), sentinel, dtype=torch.int32, device=dev)
    pick_actions(mode, None if probs is None else torch.from_numpy(probs).to(dev), None if valid is None else torch.from_numpy(valid).to(dev),
                 None if active is None else torch.from_numpy(active).to(dev), rng_seed=SEED, stream0=stream0, counters=cnt, out=out)
    return out.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize('T', [1, 3, 65])
@pytest.mark.parametrize('A', [21, 81, 3402])
def test_modes_equal_the_numpy_restatement(A, T):
    pats = row_patterns(A)
    assert len(pats) < 65                                  # (65 rows walk through every pattern; 1 and 3 start at different ones)
    rows = [pats[(i + A + T) % len(pats)] for i in range(T)]
    probs, valid = np.stack([p for _, p, _ in rows]), np.stack([v for _, _, v in rows])
    u_all = draws(STREAM0, 0, T, N_SEARCH)
    counters = np.array([int(np.argmax(u_all[i])) if rows[i][0] == 'u_near_1' else 3 * i + 1 for i in range(T)], dtype=np.int64)
    u = u_all[np.arange(T), counters]
    for i in range(T):
        if rows[i][0] == 'u_near_1':
            assert u[i] > 0.99, u[i]
    for mode in (0, 1, 2):
        got, cnt = run(mode, probs, valid, counters, sentinel=-7)
        exp = np.array([ref_pick(mode, probs[i], valid[i], u[i]) for i in range(T)])
        print('A=%d T=%d mode=%d rows=%s got=%s' % (A, T, mode, [n for n, _, _ in rows][:16], got[:16]))
        assert np.array_equal(got, exp), [(rows[i][0], int(got[i]), int(exp[i])) for i in np.flatnonzero(got != exp)]
        assert np.array_equal(cnt, counters + (0 if mode == 1 else 1)), mode
        for i in range(T):                                # whatever the mode: never an invalid action where a valid one exists
            assert valid[i, got[i]] or not valid[i].any(), (mode, rows[i][0], got[i])
    named = {n: i for i, (n, _, _) in enumerate(rows)}
    got1, _ = run(1, probs, valid, counters)
    if 'tie_5_%d' % (70 if A > 70 else A - 1) in named:
        assert got1[named['tie_5_%d' % (70 if A > 70 else A - 1)]] == 5
    if 'all_nan' in named:
        assert got1[named['all_nan']] == 0
    if 'none_valid' in named:
        for mode in (0, 1, 2):
            assert run(mode, probs, valid, counters, sentinel=-7)[0][named['none_valid']] == 0


def test_inactive_games_keep_their_action_and_counter():
    T, A = 65, 81
    pats = row_patterns(A)
    probs, valid = np.stack([pats[i % len(pats)][1] for i in range(T)]), np.stack([pats[i % len(pats)][2] for i in range(T)])
    active = (np.arange(T) % 3 != 0).astype(np.uint8)
    counters = np.arange(T, dtype=np.int64) * 5 + 2
    u = draws(STREAM0, 0, T, int(counters.max()) + 1)[np.arange(T), counters]
    for mode in (0, 1, 2):
        got, cnt = run(mode, probs, valid, counters, active=active, sentinel=-7)
        exp = np.array([ref_pick(mode, probs[i], valid[i], u[i]) if active[i] else -7 for i in range(T)])
        assert np.array_equal(got, exp), mode
        assert np.array_equal(cnt, counters + (active if mode != 1 else 0)), mode


def test_two_launches_from_the_same_counters_pick_the_same():
    T, A = 65, 3402
    r = np.random.RandomState(7)
    probs = (r.randint(0, 1 << 16, size=(T, A)) / 65536.0).astype(np.float32)
    valid = (r.rand(T, A) < 0.2).astype(np.uint8)
    counters = r.randint(0, 1000, size=T).astype(np.int64)
    for mode in (0, 2):
        a, ca = run(mode, probs, valid, counters)
        b, cb = run(mode, probs, valid, counters)
        assert np.array_equal(a, b) and np.array_equal(ca, cb) and np.array_equal(ca, counters + 1)
        assert valid[np.arange(T), a].all()


def test_argmax_without_a_mask_is_the_arena_selection():
    """valid = None, mode 1: the torch expression BatchedArena.play_wave applies to getActionProb's rows (first index of the row maximum,
    0 when no entry equals it), on 256 rows whose maxima are duplicated"""
    import torch
    from azg_amd.arena import pick_actions
    T, A = 256, 81
    r = np.random.RandomState(11)
    probs = torch.from_numpy((r.randint(0, 8, size=(T, A)) / 8.0).astype(np.float32)).cuda()
    assert int(((probs == probs.max(dim=1, keepdim=True).values).sum(dim=1) > 1).sum()) > T // 2
    ar = torch.arange(A, device=probs.device)[None, :]
    first_max = torch.where(probs == probs.max(dim=1, keepdim=True).values, ar, A).min(dim=1).values
    first_max = torch.where(first_max >= A, torch.zeros_like(first_max), first_max)
    got = pick_actions(1, probs, None)
    assert torch.equal(got, first_max.to(torch.int32))


def test_uniform_draws_over_successive_counters():
    """65 games x 64 successive counters on a row with 7 valid actions: every one of the 4160 picks is the restatement's (hence valid), the
    kernel's own counter walks 0..64, and every one of the 7 actions occurs.  (No chi-square threshold: each draw is pinned exactly.)"""
    T, A, N = 65, 81, 64
    valid = np.zeros((T, A), np.uint8)
    seven = np.array([2, 9, 31, 63, 64, 70, 80])
    valid[:, seven] = 1
    u = draws(STREAM0, 0, T, N)
    import torch
    from azg_amd.arena import pick_actions
    v = torch.from_numpy(valid).cuda()
    cnt = torch.zeros(T, dtype=torch.int64, device='cuda:0')
    picks = torch.stack([pick_actions(0, None, v, rng_seed=SEED, stream0=STREAM0, counters=cnt) for _ in range(N)], dim=1).cpu().numpy()
    assert np.array_equal(cnt.cpu().numpy(), np.full(T, N))
    exp = seven[np.minimum(np.floor(u * 7).astype(np.int64), 6)]
    assert np.array_equal(picks, exp)
    assert set(picks.reshape(-1).tolist()) == set(seven.tolist())


def test_sample_general_floats():
    """arbitrary f32 rows (a softmax-like spread over eight orders of magnitude): the pick is a valid action of positive probability whose
    cumulative interval contains u * total up to the difference two f64 summation orders of A terms can make (A * 2^-52, relative)"""
    T, A = 65, 3402
    r = np.random.RandomState(5)
    probs = np.exp(r.uniform(-18, 0, size=(T, A))).astype(np.float32)
    valid = (r.rand(T, A) < 0.5).astype(np.uint8)
    counters = np.arange(T, dtype=np.int64)
    u = draws(STREAM0, 0, T, T)[np.arange(T), counters]
    got, _ = run(2, probs, valid, counters)
    eps = A * 2.0 ** -52
    for i in range(T):
        w = np.where(valid[i] != 0, probs[i], 0).astype(np.float64)
        cum = np.cumsum(w)
        a, target = int(got[i]), u[i] * cum[-1]
        assert valid[i, a] and probs[i, a] > 0
        assert cum[a] >= target * (1 - eps) and cum[a] - w[a] <= target * (1 + eps), (i, a, cum[a] - w[a], target, cum[a])


def test_refused_inputs():
    import torch
    from azg_amd import AzgError
    from azg_amd.arena import pick_actions
    valid = torch.ones((3, 21), dtype=torch.uint8, device='cuda:0')
    probs = torch.ones((3, 21), dtype=torch.float32, device='cuda:0')
    for mode in (-1, 3):
        with pytest.raises(AzgError):
            pick_actions(mode, probs, valid)
    for mode in (1, 2):
        with pytest.raises(AzgError):
            pick_actions(mode, None, valid)
    out = pick_actions(0, probs[:0], valid[:0])                      # T == 0: nothing is launched
    assert out.shape == (0,)
    torch.cuda.synchronize()
