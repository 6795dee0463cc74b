"""Weight sets for the engine nets other than the shipped checkpoints (a helper module of tests/test_net_weight_sets.py and
tests/test_gpu_net_weight_sets.py, not a conftest; tests/reachboards.py and its tests use the calibrated set, the float64 reference and
the operand forms / evaluator factory at the end of this file).

Every row of nnet_wrapper.ENGINE_NETS is held on two weight sets made from seeds at test time:

  fresh(config, seed)       the trainable module as constructed (what a Coach run without a checkpoint starts from: BatchNorm statistics
                            0 / 1, gains 1, BatchNorm / LayerNorm / attention biases 0);
  calibrated(config, seed)  fresh, with running means and variances, zero-initialised tensors and all-ones gains set to non-trivial
                            values (a third of the gains negative), plus amp[k] * delta[k] on every floating tensor k.  delta comes from a
                            seeded CPU generator; amp from tests/golden/netweights_amplitudes.json, which calibrate() writes: it doubles a
                            tensor's amplitude (AMP0 up to AMP_CAP) until removing that tensor's perturbation moves the float64 output by
                            a margin over what the CPU test asks (test_net_weight_sets.py::test_every_tensor_counts).

The reference of both is the module itself in float64 (float64_outputs): a deep copy in double with a forward pre-hook on every leaf
module that casts floating inputs to double (the modules' forwards call boards.float()).

Regenerate the table with  python tests/netweights.py  (CPU only; the file must come out unchanged)."""
import collections
import copy
import functools
import json
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
AMPLITUDES = os.path.join(GOLDEN, 'netweights_amplitudes.json')
SEED = 1                       # the seed the amplitude table was calibrated for (the tests use it) ...
# ... except where the seed-1 calibrated set saturates v (|v| >= 0.999) on more than half the fixture rows, which would hide the value
# head from a 1e-5 bound (test_net_weight_sets.py::test_outputs_are_not_degenerate)
SEEDS = {'akropolis3_v31': 2, 'tlp3_v83': 2}
AMP0, AMP_CAP = 0.25, 8.0      # a perturbation of 25 % of a tensor's rms, doubled up to 32 x
CONTRACT = 1e-5                # include/azg.h: the kernels' distance from the f64 forward of the same weights
VAR_LOG = (-0.7, 2.1)          # running variances: log-uniform in [1/2, 8]
LOO_BOARDS = 4                 # boards of the leave-one-out pass (calibration and test)

# tag -> {tensor name: why its leave-one-out effect may stay below the bound of test_every_tensor_counts}; at most two per net
EXCUSED = {}

Config = collections.namedtuple('Config', 'row game args tag')


def _rows():
    from azg_amd import _lib, nnet_wrapper
    by = {(r.game, r.version): r for r in nnet_wrapper.ENGINE_NETS}
    return _lib, by


def configs():
    """every (ENGINE_NETS row, game constructor -- the games.<class> name and its arguments, so that listing needs no GPU --, fixture
    tag) with boards in tests/golden/netfwd_<tag>.npz, as Config(row, game, args, tag)"""
    L, by = _rows()
    out = [Config(by[L.SPLENDOR, 80], 'SplendorGame', (p,), 'splendor%d_v80' % p) for p in (2, 3, 4)]
    out += [Config(by[L.AZUL, 84], 'AzulGame', (), 'azul_v84'),
            Config(by[L.SANTORINI, 89], 'SantoriniGame', (1,), 'santorini1_v89'),
            Config(by[L.SANTORINI, 78], 'SantoriniGame', (11,), 'santorini11_v78'),
            Config(by[L.ABALONE, 21], 'AbaloneGame', (), 'abalone_v21')]
    out += [Config(by[L.SMALLWORLD, 62], 'SmallworldGame', (p,), 'smallworld%s_v62' % ('' if p == 2 else p)) for p in (2, 3, 4)]
    out += [Config(by[L.AKROPOLIS, 31], 'AkropolisGame', (p,), 'akropolis%s_v31' % ('' if p == 2 else p)) for p in (2, 3, 4)]
    out += [Config(by[L.MINIVILLES, 82], 'MinivillesGame', (p,), 'minivilles%d_v82' % p) for p in (2, 3, 4)]
    out += [Config(by[L.TLP, 83], 'TLPGame', (p,), 'tlp%d_v83' % p) for p in (3, 4, 5)]
    out += [Config(by[L.BOTANIK, v], 'BotanikGame', (), 'botanik_v%d' % v) for v in (10, 11)]
    return out


def config(tag):
    return next(c for c in configs() if c.tag == tag)


def game(cfg):
    """the engine's game object (needs the built library and a GPU)"""
    from azg_amd import games
    return getattr(games, cfg.game)(*cfg.args)


@functools.lru_cache(maxsize=None)
def _fixture(tag):
    d = np.load(os.path.join(GOLDEN, 'netfwd_%s.npz' % tag))
    return d['boards'], d['masks']


def shape(cfg):
    """(P, A) read off the fixture, so that nothing here needs the built library"""
    d = np.load(os.path.join(GOLDEN, 'netfwd_%s.npz' % cfg.tag))
    return int(d['v'].shape[1]), int(d['masks'].shape[1])


def raw_boards(tag, B):
    """the first B fixture rows (tiled if the fixture is shorter), unedited: boards int8 [B, ...], masks uint8 [B, A]"""
    b, m = _fixture(tag)
    rows = np.arange(B) % len(b)
    return torch.from_numpy(b[rows].copy()), torch.from_numpy(m[rows].copy())


def boards(tag, B):
    """raw_boards with edited masks in the last two rows: row B - 2 has no valid action (the reference gives uniform pi), row B - 1
    exactly one (the first valid action of its fixture row, action 0 if it had none)"""
    b, m = raw_boards(tag, B)
    assert B >= 2
    m[B - 2] = 0
    one = int(m[B - 1].argmax())
    m[B - 1] = 0
    m[B - 1, one] = 1
    return b, m


def loo_boards(tag, B=LOO_BOARDS):
    """the boards of the leave-one-out pass: the B fixture rows with the most valid actions (ties: the earlier row), each mask thinned
    to three of them (the first, the middle and the last valid action).  A row with one valid action has pi = 1 whatever the policy head
    computes (the first rows of the Minivilles and Little Prince fixtures), and with n valid actions of similar logits a change d of a
    logit moves pi by about d / n only: three valid actions, spread over the action layout, show a policy tensor best.  The GPU test
    evaluates these rows too, so what is proved on them holds for its batch"""
    b, m = _fixture(tag)
    rows = np.sort(np.argsort(-m.sum(axis=1).astype(np.int64), kind='stable')[:B])
    b, m = b[rows].copy(), m[rows].copy()
    for r in range(B):
        valid = np.flatnonzero(m[r])
        m[r] = 0
        m[r, valid[[0, len(valid) // 2, len(valid) - 1]]] = 1
    return torch.from_numpy(b), torch.from_numpy(m)


def gpu_boards(tag, B=70):
    """the batch of the GPU test: boards(tag, B - LOO_BOARDS) followed by loo_boards(tag)"""
    b, m = boards(tag, B - LOO_BOARDS)
    lb, lm = loo_boards(tag)
    return torch.cat([b, lb]), torch.cat([m, lm])


def seed_of(cfg):
    return SEEDS.get(cfg.tag, SEED)


def fresh(cfg, seed=None):
    """the module as constructed under torch.manual_seed(seed) (the global generator is restored), dropout 0, eval()"""
    P, A = shape(cfg)
    seed = seed_of(cfg) if seed is None else seed
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        m = cfg.row.module(P, A, 0.0)
    return m.eval()


def tensors(module):
    """name -> tensor of every floating state_dict entry except `lowvalue` (the perturbed / counted tensors)"""
    return {k: t for k, t in module.state_dict().items() if t.is_floating_point() and k != 'lowvalue'}


@functools.lru_cache(maxsize=None)
def amplitudes():
    with open(AMPLITUDES) as f:
        return json.load(f)


def _detrivialise_and_deltas(module, seed):
    """in place: running statistics, zero-initialised tensors and all-ones gains of `module` get non-trivial values; -> name -> delta
    (the unit perturbation of each tensor: its rms times a standard normal; for a running variance a non-negative multiple of itself, so
    that any amplitude keeps it positive)"""
    g = torch.Generator().manual_seed(1000003 * seed + 17)
    randn = lambda t: torch.randn(t.shape, generator=g, dtype=torch.float32)  # noqa: E731
    rand = lambda t: torch.rand(t.shape, generator=g, dtype=torch.float32)  # noqa: E731
    deltas = {}
    with torch.no_grad():
        for k, t in tensors(module).items():
            if k.endswith('running_mean'):
                t.copy_(0.5 * randn(t))
            elif k.endswith('running_var'):
                t.copy_(torch.exp(VAR_LOG[0] + (VAR_LOG[1] - VAR_LOG[0]) * rand(t)))  # log-uniform
            elif bool((t == 0).all()):
                t.copy_(0.1 * randn(t))
            elif bool((t == 1).all()):
                t.copy_((0.5 + rand(t)) * torch.where(rand(t) < 1.0 / 3.0, -1.0, 1.0))
            if k.endswith('running_var'):
                deltas[k] = t.detach().clone() * rand(t)
            else:
                rms = float(t.detach().double().pow(2).mean().sqrt())
                deltas[k] = max(rms, 1e-3) * randn(t)
    return deltas


def _perturbed(cfg, seed, amp):
    """(module with every tensor at base + amp * delta, name -> the tensor's base value)"""
    seed = seed_of(cfg) if seed is None else seed
    m = fresh(cfg, seed)
    deltas = _detrivialise_and_deltas(m, seed)
    base = {}
    with torch.no_grad():
        for k, t in tensors(m).items():
            base[k] = t.detach().clone()
            t.add_(float(amp[k]) * deltas[k])
    return m, base


def calibrated(cfg, seed=None, without=None):
    """the calibrated weight set; `without`: a tensor name whose perturbation is left out (the leave-one-out nets of the CPU test)"""
    m, base = _perturbed(cfg, seed, amplitudes()[cfg.tag])
    if without is not None:
        with torch.no_grad():
            tensors(m)[without].copy_(base[without])
    return m


WEIGHT_SETS = {'fresh': fresh, 'calibrated': calibrated}


def _cast_inputs(mod, args):
    return tuple(a.double() if torch.is_tensor(a) and a.is_floating_point() else a for a in args)


def _double_copy(module):
    m = copy.deepcopy(module).double().eval()
    for sub in m.modules():
        if not list(sub.children()):
            sub.register_forward_pre_hook(_cast_inputs)
    return m


def _forward(m, b, k):
    dev = next(m.parameters()).device
    # (grad mode stays on: nn.TransformerEncoderLayer then takes its plain-op path, in f32 and in f64 alike)
    log_pi, v = m(b.to(dev), k.to(dev).bool())
    return torch.exp(log_pi.detach()), v.detach()


def float64_outputs(module, b, k):
    """(exp(log_pi), v) of a deep copy of `module` in double, on the module's device"""
    return _forward(_double_copy(module), b, k)


def float32_outputs(module, b, k):
    """(exp(log_pi), v) of the module as it is (f32, eval mode), as doubles"""
    pi, v = _forward(module.eval(), b, k)
    return pi.double(), v.double()


def float64_outputs_and_max_activation(module, b, k, chunk=None):
    """(exp(log_pi), v, the largest |output| of any submodule) of one float64 forward, `chunk` rows at a time (None: all at once)"""
    m = _double_copy(module)
    top = [0.0]

    def rec(mod, args, out):
        for t in (out if isinstance(out, (tuple, list)) else (out,)):
            if torch.is_tensor(t) and t.is_floating_point() and t.numel():
                top[0] = max(top[0], float(t.detach().abs().max()))
    for sub in m.modules():
        if sub is not m:
            sub.register_forward_hook(rec)
    n = len(b)
    outs = [_forward(m, b[lo:lo + (chunk or n)], k[lo:lo + (chunk or n)]) for lo in range(0, n, chunk or n)]
    return torch.cat([p for p, _ in outs]), torch.cat([v for _, v in outs]), top[0]


def max_activation(module, b, k):
    """the largest |output| of any submodule in the float64 forward"""
    return float64_outputs_and_max_activation(module, b, k)[2]


def leave_one_out(cfg, seed=None, amp=None, B=LOO_BOARDS):
    """-> (f32 error, {tensor name: effect}) of the calibrated net on loo_boards(tag, B): the error is max |f32 - f64| over pi and v, a
    tensor's effect max(max |d pi|, max |d v|) between the float64 outputs with and without that tensor's perturbation"""
    m, base = _perturbed(cfg, seed, amplitudes()[cfg.tag] if amp is None else amp)
    b, k = loo_boards(cfg.tag, B)
    p32, v32 = float32_outputs(m, b, k)
    d = _double_copy(m)
    p64, v64 = _forward(d, b, k)
    err = max(float((p32 - p64).abs().max()), float((v32 - v64).abs().max()))
    effects = {}
    dt = tensors(d)
    with torch.no_grad():
        for name, t in dt.items():
            keep = t.clone()
            t.copy_(base[name].double())
            p, v = _forward(d, b, k)
            t.copy_(keep)
            effects[name] = max(float((p - p64).abs().max()), float((v - v64).abs().max()))
    return err, effects


def bound(err):
    """what test_every_tensor_counts asks of every tensor's effect: ten times what the GPU test allows a kernel"""
    return 10.0 * (CONTRACT + err)


def calibrate(cfg, seed=None, passes=10, log=None):
    """the amplitude table of one config: every tensor starts at AMP0; a tensor whose leave-one-out effect is below 1.5 x bound (and
    3e-4) is doubled, up to AMP_CAP, for at most `passes` passes"""
    amp = {k: AMP0 for k in tensors(fresh(cfg, seed))}
    for n in range(passes):
        err, eff = leave_one_out(cfg, seed, amp)
        want = max(3e-4, 1.5 * bound(err))
        low = [k for k, e in eff.items() if e < want]
        if log:
            log('%s pass %d: f32 error %.2e, %d of %d tensors below %.2e (smallest %.2e)' % (cfg.tag, n, err, len(low), len(eff), want,
                                                                                              min(eff.values())))
        grow = [k for k in low if amp[k] < AMP_CAP]
        if not grow:
            break
        for k in grow:
            amp[k] = min(AMP_CAP, 2.0 * amp[k])
    return amp


def write_table(path=AMPLITUDES, log=print):
    """calibrate every config and write the table.  One thread: a doubling decided at a threshold must not depend on how many threads
    share an f32 sum on the machine that regenerates the file"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        table = {cfg.tag: calibrate(cfg, log=log) for cfg in configs()}
    finally:
        torch.set_num_threads(threads)
    with open(path, 'w') as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write('\n')


def base_class(cfg):
    """the plain-torch nnet.* net the row's evaluator is built on (the `base` argument of the table's factories; Splendor's factory
    builds on nnet.SplendorV80 at every player count) and whether it takes num_players: the factory's `base` / `takes_num_players`
    attributes"""
    f = cfg.row.evaluator
    return f.base, bool(f.takes_num_players)


def base_net(cfg, module, device='cpu', dtype=torch.float32):
    cls, takes_p = base_class(cfg)
    sd = {k: v.detach().cpu() for k, v in module.state_dict().items()}
    kw = dict(num_players=shape(cfg)[0]) if takes_p else {}
    return cls(sd, device=device, dtype=dtype, **kw)


MB1D = ('splendor', 'azul', 'minivilles', 'tlp')    # the tags evaluated by the MobileNet-1d kernel (Splendor 2p: by the V80 kernel too)


def forms(cfg):
    """the operand forms of a config's net: 'default' is evaluator_for's, the others name constructor arguments"""
    tag = cfg.tag
    if tag == 'splendor2_v80':
        return ['default', 'v80-bf16x3', 'v80-f32', 'mb1d-h2', 'mb1d-f32']
    if tag.startswith(MB1D):
        return ['default', 'mb1d-f32']
    if tag == 'santorini1_v89':
        return ['default', 'split', 'f32']
    if tag == 'santorini11_v78':
        return ['default', 'split', 'f32', 'h2-policy1']
    return ['default']


@functools.lru_cache(maxsize=None)
def _game(cfg):
    return game(cfg)


def evaluator(cfg, form, module, max_batch, device='cuda:0'):
    """the engine-kernel evaluator of `module`'s weights in one of forms(cfg) (needs the built library and a GPU)"""
    from azg_amd import nnet
    from azg_amd.nnet_wrapper import evaluator_for
    if form == 'default':
        return evaluator_for(module, _game(cfg), max_batch)
    sd = {k: v.detach().cpu() for k, v in module.state_dict().items()}
    if form.startswith('v80-'):
        return nnet.SplendorV80Hip(sd, num_players=2, device=device, max_batch=max_batch, split=form == 'v80-bf16x3', h2=False)
    base = base_net(cfg, module, device=device)
    if form.startswith('mb1d-'):
        return nnet.MobileNet1dHip(base, max_batch=max_batch, h2=form == 'mb1d-h2')
    hip = nnet.SantoriniV89Hip if cfg.tag == 'santorini1_v89' else nnet.SantoriniV78Hip
    kw = {'split': dict(split=True, h2=False), 'f32': dict(split=False, h2=False), 'h2-policy1': dict(h2=True, policy2=False)}[form]
    return hip(base, max_batch=max_batch, **kw)


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    write_table(*sys.argv[1:2])
