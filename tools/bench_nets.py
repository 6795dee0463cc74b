"""µs per forward at T leaves for every evaluation path of the MobileNet-1d nets, the Santorini nets, the Abalone net, the Smallworld
nets, the Akropolis nets and the Botanik nets (HIP events, 50 forwards after warm-up), and the shipped MobileNet-1d checkpoints of every
player count."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch
from azg_amd import nnet
T = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
G = os.path.join(ROOT, 'tests', 'golden')


def timed(net, boards, valids, n=50):
    for _ in range(5):
        net.predict_batch(boards, valids)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        net.predict_batch(boards, valids)
    e.record(); e.synchronize()
    return s.elapsed_time(e) / n * 1000


for tag, mk, shape, A in [('splendor2', lambda: nnet.SplendorV80.from_npz(G + '/weights_splendor2_v80.npz', device='cuda:0'), (56, 7), 81),
                          ('splendor4', lambda: nnet.SplendorV80.from_npz(G + '/weights_splendor4_v80.npz', num_players=4, device='cuda:0'), (88, 7), 81),
                          ('azul', lambda: nnet.AzulV84.from_npz(G + '/weights_azul_v84.npz', device='cuda:0'), (23, 6), 180)]:
    base = mk()
    boards = torch.randint(0, 5, (T,) + shape, dtype=torch.int8, device='cuda:0')
    valids = (torch.rand((T, A), device='cuda:0') < 0.5).to(torch.uint8)
    valids[:, -1] = 1
    row = {'torch ops': timed(base, boards, valids.bool(), 10),
           'k_mb1d_net f32': timed(nnet.MobileNet1dHip(base, max_batch=T, fused=True, h2=False), boards, valids),
           'k_mb1d_net h2': timed(nnet.MobileNet1dHip(base, max_batch=T, fused=True, h2=True), boards, valids)}
    if tag == 'splendor2':
        row['k_v80_net'] = timed(nnet.SplendorV80Hip.from_npz(G + '/weights_splendor2_v80.npz', max_batch=T), boards, valids)
    print(tag, 'T=%d' % T, '  '.join('%s %.1f us' % kv for kv in row.items()), flush=True)

base = nnet.SantoriniV89.from_npz(G + '/weights_santorini1_v89.npz', device='cuda:0')
boards = torch.randint(-2, 5, (T, 5, 5, 3), dtype=torch.int8, device='cuda:0')
valids = (torch.rand((T, 162), device='cuda:0') < 0.5).to(torch.uint8)
valids[:, 0] = 1
print('santorini1 V89 T=%d' % T, 'torch ops (MIOpen) %.1f us' % timed(base, boards, valids.bool(), 10),
      ' k_conv5_net %.1f us' % timed(nnet.SantoriniV89Hip(base, max_batch=T), boards, valids), flush=True)

base = nnet.SantoriniV78.from_npz(G + '/weights_santorini11_v78.npz', device='cuda:0')
Tg = min(T, 1024)
boards = torch.randint(-2, 5, (Tg, 5, 5, 3), dtype=torch.int8, device='cuda:0')
valids = (torch.rand((Tg, 1782), device='cuda:0') < 0.1).to(torch.uint8)
valids[:, 0] = 1
print('santorini11 V78 T=%d' % Tg, 'torch ops (MIOpen) %.1f us' % timed(base, boards, valids.bool(), 5),
      ' k_s78_net %.1f us' % timed(nnet.SantoriniV78Hip(base, max_batch=Tg), boards, valids), flush=True)

# Abalone V21 at T: the plain-torch net (BN folded), the one-launch kernel, and the trainable module through TorchModuleEvaluator (the path
# of a game without an engine net: BN unfolded, log_softmax + exp)
from azg_amd import games, train  # noqa: E402
import numpy as np  # noqa: E402
base = nnet.AbaloneV21.from_npz(G + '/weights_abalone_v21.npz', device='cuda:0')
d = np.load(G + '/netfwd_abalone_v21.npz')
idx = np.arange(T) % len(d['boards'])
boards = torch.from_numpy(d['boards'][idx].reshape(T, -1)).to('cuda:0')
valids = torch.from_numpy(d['masks'][idx]).to('cuda:0')
z = np.load(G + '/weights_abalone_v21.npz')
mod = train.AbaloneV21Module()
mod.load_state_dict({k[3:]: torch.as_tensor(z[k]) for k in z.files if k.startswith('sd/')}, strict=True)
print('abalone V21 T=%d' % T, 'torch ops (MIOpen) %.1f us' % timed(base, boards, valids.bool(), 10),
      ' k_aba21_net %.1f us' % timed(nnet.AbaloneV21Hip(base, max_batch=T), boards, valids),
      ' TorchModuleEvaluator %.1f us' % timed(nnet.TorchModuleEvaluator(mod, games.AbaloneGame()), boards, valids, 10), flush=True)

# Smallworld V62 at T for 2, 3 and 4 players: the plain-torch net (stem folded), the one-launch kernel, and the trainable module through
# TorchModuleEvaluator (the path of a game without an engine net: nn.TransformerEncoder, log_softmax + exp)
for P, tag in ((2, 'smallworld_v62'), (3, 'smallworld3_v62'), (4, 'smallworld4_v62')):
    base = nnet.SmallworldV62.from_npz(G + '/weights_%s.npz' % tag, num_players=P, device='cuda:0')
    d = np.load(G + '/netfwd_%s.npz' % tag)
    idx = np.arange(T) % len(d['boards'])
    boards = torch.from_numpy(d['boards'][idx].reshape(T, -1)).to('cuda:0')
    valids = torch.from_numpy(d['masks'][idx]).to('cuda:0')
    z = np.load(G + '/weights_%s.npz' % tag)
    mod = train.SmallworldV62Module(P, base.A)
    mod.load_state_dict({k[3:]: torch.as_tensor(z[k]) for k in z.files if k.startswith('sd/')}, strict=True)
    print('smallworld%d V62 T=%d' % (P, T), 'torch ops %.1f us' % timed(base, boards, valids.bool(), 10),
          ' k_sw62_net %.1f us' % timed(nnet.SmallworldV62Hip(base, max_batch=T), boards, valids),
          ' TorchModuleEvaluator %.1f us' % timed(nnet.TorchModuleEvaluator(mod, games.SmallworldGame(P)), boards, valids, 10), flush=True)

# Akropolis V31 at T for 2, 3 and 4 players: the plain-torch net (BatchNorms folded, einsum policy), the one-launch kernel, and the
# trainable module through TorchModuleEvaluator (the reference's algorithm, its policy product summed by einsum), on random int8 boards
# with random masks.  Floors from shapes: the reference's multiply-adds per sample (conv 5 -> 8 and 8 -> 8 per player, proj_p's
# 1x1 (8P + 24 -> 32), depthwise and project, the 169 x 16 x 6 CS policy product) at the f32 peak (157.3 TF), and the HBM bytes
# (boards, valid, pi, v) at 8 TB/s; the kernel's share is the larger floor over its time.
for P, tag in ((2, 'akropolis_v31'), (3, 'akropolis3_v31'), (4, 'akropolis4_v31')):
    CS, C = P + 2, 3 * P + 2
    S, A = 169 * C, 1014 * CS
    mac = P * 169 * 8 * (5 * 9 + 8 * 9) + 169 * 32 * (8 * P + 24) + 169 * 32 + 169 * 16 * 32 + CS * 6 * 169 * 16
    t_flop = 2.0 * mac * T / 157.3e12 * 1e6
    t_hbm = (S + A + 4 * A + 4 * P) * T / 8.0e12 * 1e6
    base = nnet.AkropolisV31.from_npz(G + '/weights_%s.npz' % tag, num_players=P, device='cuda:0')
    gen = torch.Generator(device='cuda:0').manual_seed(P)
    boards = torch.randint(-128, 128, (T, S), dtype=torch.int8, device='cuda:0', generator=gen)
    valids = (torch.rand((T, A), device='cuda:0', generator=gen) < 0.1).to(torch.uint8)
    valids[:, 0] = 1
    z = np.load(G + '/weights_%s.npz' % tag)
    mod = train.AkropolisV31Module(P, A)
    mod.load_state_dict({k[3:]: torch.as_tensor(z[k]) for k in z.files if k.startswith('sd/')}, strict=True)
    t_k = timed(nnet.AkropolisV31Hip(base, max_batch=T), boards, valids)
    print('akropolis%d V31 T=%d' % (P, T), 'torch ops %.1f us' % timed(base, boards, valids.bool(), 10), ' k_akr31_net %.1f us' % t_k,
          ' TorchModuleEvaluator %.1f us' % timed(nnet.TorchModuleEvaluator(mod, games.AkropolisGame(P)), boards, valids, 10),
          ' floors: %.1f MFLOP/sample = %.1f us at the f32 peak, %.1f MB = %.1f us at 8 TB/s;  kernel at %.0f %% of the %s floor'
          % (2e-6 * mac, t_flop, (S + 5 * A + 4 * P) * T / 1e6, t_hbm, 100 * max(t_flop, t_hbm) / t_k, 'compute' if t_flop >= t_hbm else 'HBM'),
          flush=True)

# The shipped MobileNet-1d checkpoints the one-launch kernel runs at their own geometries (Splendor 3p, Minivilles 3 / 4p, The Little Prince
# 4 / 5p): the plain-torch net, k_mb1d_net f32 and h2, on the fixture boards tiled to T.  Floors from shapes: multiply-adds per sample (first
# layer L C^2; per block expand and project 2 L C E, token mix L^2 E, SE 2 E Q; heads L C (A + P) + A^2 + P^2) at the f32 peak (157.3 TF),
# and the HBM bytes (f32 weights once, int8 boards, u8 valid, f32 pi and v) at 8 TB/s; the kernel's share is the larger floor over its time.
for tag in ('splendor3_v80', 'minivilles3_v82', 'minivilles4_v82', 'tlp4_v83', 'tlp5_v83'):
    from azg_amd import formats   # (Minivilles 4p: the stand-in weights of the same shapes, weightstats_minivilles4_v82.npz)
    sd = formats.fixture_state_dict(G, tag)[0]
    base = nnet.MobileNet1d(sd, device='cuda:0')
    L, C, A, P = base.L, base.nb_vect, base.A, base.P
    blocks = (base.trunk, base.head_pi, base.head_v)
    mac = L * C * C + sum(2 * L * C * b.We.shape[1] + L * L * b.We.shape[1] + 2 * b.We.shape[1] * b.W1.shape[1] for b in blocks) \
        + L * C * (A + P) + A * A + P * P
    n_w = sum(int(np.prod(v.shape)) for v in sd.values())
    t_flop = 2.0 * mac * T / 157.3e12 * 1e6
    hbm = 4 * n_w + (C * L + A + 4 * A + 4 * P) * T
    t_hbm = hbm / 8.0e12 * 1e6
    d = np.load(G + '/netfwd_%s.npz' % tag)
    idx = np.arange(T) % len(d['boards'])
    boards = torch.from_numpy(d['boards'][idx].reshape(T, -1)).to('cuda:0')
    valids = torch.from_numpy(d['masks'][idx]).to('cuda:0')
    t32 = timed(nnet.MobileNet1dHip(base, max_batch=T, h2=False), boards, valids)
    th2 = timed(nnet.MobileNet1dHip(base, max_batch=T, h2=True), boards, valids)
    print('%s T=%d' % (tag, T), 'torch ops %.1f us' % timed(base, boards, valids.bool(), 10), ' k_mb1d_net f32 %.1f us' % t32,
          ' k_mb1d_net h2 %.1f us' % th2,
          ' floors: %.2f MFLOP/sample = %.1f us at the f32 peak, %.1f MB = %.1f us at 8 TB/s;  h2 kernel at %.0f %% of the %s floor'
          % (2e-6 * mac, t_flop, hbm / 1e6, t_hbm, 100 * max(t_flop, t_hbm) / th2, 'compute' if t_flop >= t_hbm else 'HBM'), flush=True)

# Botanik V10 / V11 (no checkpoint: the stand-in weights of weightstats_botanik_v1x.npz) at T: the plain-torch net, the one-launch kernel
# and the trainable module through TorchModuleEvaluator, on the fixture boards tiled to T.  Floors from shapes: multiply-adds per sample
# (1-d branch: first layer 30*7*7, per block 2*30*7*21 + 30*30*21 + 2*21*8, FC 210*430; per machine branch: conv 49*63*16, trunk
# 2*49*16*32 + 49*32*9, six head blocks 2*49*16*48 + 49*48*9 + 2*48*16, FC 784*430; final 2*428^2 + 2*2^2) at the f32 peak (157.3 TF),
# and the HBM bytes (f32 weights once, int8 boards, u8 valid, f32 pi and v) at 8 TB/s; the kernel's share is the larger floor over its time.
for version in (10, 11):
    from azg_amd import formats
    tag = 'botanik_v%d' % version
    sd = formats.fixture_state_dict(G, tag)[0]
    base = nnet.BotanikV1x(sd, device='cuda:0')
    M = base.n_mach
    mac = 30 * 49 + 3 * (2 * 30 * 7 * 21 + 30 * 30 * 21 + 2 * 21 * 8) + 210 * 430 \
        + M * (49 * 63 * 16 + 2 * 49 * 16 * 32 + 49 * 32 * 9 + 6 * (2 * 49 * 16 * 48 + 49 * 48 * 9 + 2 * 48 * 16) + 784 * 430) + 2 * 428 * 428 + 8
    n_w = sum(int(np.prod(v.shape)) for v in sd.values())
    t_flop = 2.0 * mac * T / 157.3e12 * 1e6
    hbm = 4 * n_w + (2310 + 428 + 4 * 428 + 8) * T
    t_hbm = hbm / 8.0e12 * 1e6
    d = np.load(G + '/netfwd_%s.npz' % tag)
    idx = np.arange(T) % len(d['boards'])
    boards = torch.from_numpy(d['boards'][idx].reshape(T, -1)).to('cuda:0')
    valids = torch.from_numpy(d['masks'][idx]).to('cuda:0')
    mod = (train.BotanikV10Module if version == 10 else train.BotanikV11Module)()
    mod.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    t_k = timed(nnet.BotanikV1xHip(base, max_batch=T), boards, valids)
    print('botanik V%d T=%d' % (version, T), 'torch ops %.1f us' % timed(base, boards, valids.bool(), 10), ' k_bot_net %.1f us' % t_k,
          ' TorchModuleEvaluator %.1f us' % timed(nnet.TorchModuleEvaluator(mod, games.BotanikGame()), boards, valids, 10),
          ' floors: %.2f MFLOP/sample = %.1f us at the f32 peak, %.1f MB = %.1f us at 8 TB/s;  kernel at %.0f %% of the %s floor'
          % (2e-6 * mac, t_flop, hbm / 1e6, t_hbm, 100 * max(t_flop, t_hbm) / t_k, 'compute' if t_flop >= t_hbm else 'HBM'), flush=True)
