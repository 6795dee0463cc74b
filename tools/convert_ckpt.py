"""Convert a reference checkpoint (.pt with pickled full_model, needs torchvision) into plain tensors + MCTS args, and
record net-forward golden vectors (G4) from the reference's own model.  Build-container only.
    python tools/convert_ckpt.py
    python tools/convert_ckpt.py --botanik          (the Botanik stand-in fixtures, below)
writes tests/golden/weights_splendor2_v80.npz (state_dict tensors + embedded MCTS args, DATA only) and
       tests/golden/netfwd_splendor2_v80.npz (256 boards/masks -> the reference model's pi, v)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'refshim'))
import harness as H  # noqa: E402

GOLDEN = os.path.join(HERE, '..', 'tests', 'golden')
# checkpoints whose weights are too large to keep as a fixture (Minivilles 4p: 1.3 MB of f32 that does not compress): the fixture is
# weightstats_<tag>.npz (shapes and per-tensor statistics, azg_amd.formats.weight_stats) and the forward vectors are the reference
# module's outputs on the stand-in weights drawn from it (formats.synthetic_state_dict)
STANDIN = {'minivilles4_v82': 4}
# tags whose boards do not come from env_<first word of the tag>.npz: the nets of Abalone's two other layouts take the positions of their own
# layout (tools/gen_golden_abalone_variants.py), the classic one -- trained with dynamic komi -- boards that carry the komi bit
ENV_OF = {'abalone_v21_german': 'abalone_german', 'abalone_v21_classic': 'abalone_classic_komi'}


def _standin(name, model):
    """load the stand-in weights of weightstats_<name>.npz into the reference's module (strict: every key, every shape)"""
    import torch
    sys.path.insert(0, os.path.join(HERE, '..'))
    from azg_amd import formats
    sd = formats.synthetic_state_dict(np.load(os.path.join(GOLDEN, 'weightstats_%s.npz' % name)))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model


def convert(name, ckpt_rel, load_kw, game_mod, game_cls, n_vec=256, forward=True):
    import torch
    m = H.load_reference(**load_kw)
    ck = torch.load(os.path.join(H.REFERENCE, ckpt_rel), map_location='cpu', weights_only=False)
    sd = {k: v.numpy() for k, v in ck['state_dict'].items()}
    meta = {k: ck[k] for k in ck if k not in ('state_dict', 'full_model')}
    if name in STANDIN:
        sys.path.insert(0, os.path.join(HERE, '..'))
        from azg_amd import formats
        out = formats.weight_stats(sd, seed=STANDIN[name])
    else:
        out = {'sd/' + k: v for k, v in sd.items()}
    for k, v in meta.items():
        if isinstance(v, (int, float, bool)):
            out['arg/' + k] = np.array(v)
        elif isinstance(v, (list, tuple)) and all(isinstance(x, (int, float)) for x in v):
            out['arg/' + k] = np.array(v, dtype=np.float64)
    H.savez(os.path.join(GOLDEN, '%s_%s.npz' % ('weightstats' if name in STANDIN else 'weights', name)), **out)
    print(name, 'args:', {k: v for k, v in meta.items() if k in ('nn_version', 'cpuct', 'fpu', 'universes', 'numMCTSSims',
                                                                   'dirichletAlpha', 'temperature', 'tempThreshold')})
    if not forward:      # the pickled full_model needs the real torchvision (absent here): weights + args only
        print('wrote weights for', name, '(no forward vectors)')
        H.cleanup()
        return
    # G4: forward vectors from the reference's own module (GenericNNetWrapper.py:112-120 torch branch)
    model = ck['full_model'].eval()
    if name in STANDIN:
        model = _standin(name, model)
    env = np.load(os.path.join(GOLDEN, 'env_%s.npz' % ENV_OF.get(name, name.split('_')[0])))
    rng = np.random.default_rng(0)
    sel = rng.choice(len(env['canonical']), size=min(n_vec, len(env['canonical'])), replace=False)
    g = getattr(m[game_mod], game_cls)()
    shape = tuple(g.getBoardSize())
    boards = env['canonical'][sel].reshape((-1,) + shape)
    masks = np.array([g.getValidMoves(b, 0) for b in boards])
    with torch.no_grad():
        lp, v = model(torch.from_numpy(boards.astype(np.float32)), torch.from_numpy(masks.astype(bool)))
    H.savez(os.path.join(GOLDEN, 'netfwd_%s.npz' % name), boards=boards.astype(np.int8),
            masks=masks.astype(np.uint8), pi=torch.exp(lp).numpy(), v=v.numpy())
    print('wrote weights +', len(sel), 'forward vectors for', name)
    H.cleanup()


def forward_f64(name, ckpt_rel, load_kw):
    """netfwd64_<name>.npz: the reference's OWN module evaluated in float64 (model.double()) on the boards / masks of
    netfwd_<name>.npz -- the rounding-free value of the reference's forward.  Evidence for the value-head tolerance: the
    reference's f32 output itself differs from it by up to ~1e-5 (printed), so the tests bound |ours - f64| <= 1e-5."""
    import torch
    H.load_reference(**load_kw)
    ck = torch.load(os.path.join(H.REFERENCE, ckpt_rel), map_location='cpu', weights_only=False)
    model = ck['full_model'].eval()
    if name in STANDIN:
        model = _standin(name, model)
    model = model.double()
    if hasattr(model, 'stem'):
        # SmallworldNNet.py InputStem.forward hard-codes .float() on the num_proj / bit_proj inputs: recast them to f64 on the way
        # in (forward pre-hooks; the reference's source stays as it is)
        for mod in (model.stem.num_proj, model.stem.bit_proj):
            mod.register_forward_pre_hook(lambda _m, args: tuple(a.double() for a in args))
    d = np.load(os.path.join(GOLDEN, 'netfwd_%s.npz' % name))
    with torch.no_grad():
        lp, v = model(torch.from_numpy(d['boards'].astype(np.float64)), torch.from_numpy(d['masks'].astype(bool)))
    pi64, v64 = torch.exp(lp).numpy(), v.numpy()
    H.savez(os.path.join(GOLDEN, 'netfwd64_%s.npz' % name), pi64=pi64, v64=v64)
    print('%-16s |ref_f32 - ref_f64|: pi %.3g  v %.3g' % (name, np.abs(d['pi'] - pi64).max(), np.abs(d['v'] - v64).max()))
    H.cleanup()


def forward_random(name, ckpt_rel, load_kw, n=16):
    """netfwdrand_<name>.npz: n boards of uniformly random int8 content (codes outside the embedding's range, negative heights and
    scores) with all-valid masks, through the reference's own module in f32 (pi, v) and in f64 (pi64, v64).  Akropolis tags only."""
    import torch
    m = H.load_reference(**load_kw)
    ck = torch.load(os.path.join(H.REFERENCE, ckpt_rel), map_location='cpu', weights_only=False)
    g = m['AkropolisGame'].AkropolisGame()
    shape, A = tuple(g.getBoardSize()), g.getActionSize()
    boards = np.random.default_rng(1).integers(-128, 128, size=(n,) + shape).astype(np.int8)
    masks = np.ones((n, A), dtype=np.uint8)
    model = ck['full_model'].eval()
    with torch.no_grad():
        lp, v = model(torch.from_numpy(boards.astype(np.float32)), torch.from_numpy(masks.astype(bool)))
        lp64, v64 = model.double()(torch.from_numpy(boards.astype(np.float64)), torch.from_numpy(masks.astype(bool)))
    out = dict(boards=boards, masks=masks, pi=torch.exp(lp).numpy(), v=v.numpy(), pi64=torch.exp(lp64).numpy(), v64=v64.numpy())
    np.savez_compressed(os.path.join(GOLDEN, 'netfwdrand_%s.npz' % name), **out)
    print('%-16s random boards |ref_f32 - ref_f64|: pi %.3g  v %.3g' % (name, np.abs(out['pi'] - out['pi64']).max(),
                                                                         np.abs(out['v'] - out['v64']).max()))
    H.cleanup()


# tag -> (checkpoint, load_reference arguments) of every netfwd64_<tag>.npz
F64 = [('splendor2_v80', 'splendor/pretrained_2players.pt', dict(splendor_players=2)),
       ('splendor4_v80', 'splendor/pretrained_4players.pt', dict(splendor_players=4)),
       ('santorini1_v89', 'santorini/pretrained.pt', dict(santorini_gods=1)),
       ('azul_v84', 'azul/pretrained.pt', dict()),
       ('santorini11_v78', 'santorini/pretrained_withgods.pt', dict(santorini_gods=11)),
       ('minivilles2_v82', 'minivilles/pretrained_2players.pt', dict(minivilles_players=2)),
       ('tlp3_v83', 'thelittleprince/pretrained_3players.pt', dict(tlp_players=3)),
       ('splendor3_v80', 'splendor/pretrained_3players.pt', dict(splendor_players=3)),
       ('minivilles3_v82', 'minivilles/pretrained_3players.pt', dict(minivilles_players=3)),
       ('minivilles4_v82', 'minivilles/pretrained_4players.pt', dict(minivilles_players=4)),
       ('tlp4_v83', 'thelittleprince/pretrained_4players.pt', dict(tlp_players=4)),
       ('tlp5_v83', 'thelittleprince/pretrained_5players.pt', dict(tlp_players=5)),
       ('abalone_v21', 'abalone/pretrained_BelgianDaisy.pt', dict()),
       ('abalone_v21_german', 'abalone/pretrained_GermanDaisy.pt', dict(abalone_layout=2)),
       ('abalone_v21_classic', 'abalone/pretrained_classic.pt', dict(abalone_layout=0, abalone_dynamic_komi=True)),
       ('smallworld_v62', 'smallworld/pretrained_2pl.pt', dict(smallworld_players=2)),
       ('smallworld3_v62', 'smallworld/pretrained_3pl.pt', dict(smallworld_players=3)),
       ('smallworld4_v62', 'smallworld/pretrained_4pl.pt', dict(smallworld_players=4)),
       ('akropolis_v31', 'akropolis/pretrained_2pl.pt', dict(akropolis_players=2)),
       ('akropolis3_v31', 'akropolis/pretrained_3pl.pt', dict(akropolis_players=3)),
       ('akropolis4_v31', 'akropolis/pretrained_4pl.pt', dict(akropolis_players=4))]


# ---- Botanik (botanik/BotanikNNet.py nn_version 10 :105-160, 11 :162-237): the reference ships no checkpoint (pretrained.pt is not in
# its snapshot), so the fixtures are stand-ins built the same way as Minivilles 4p's: the per-tensor statistics of the reference module's
# own fresh init (weightstats_botanik_v1x.npz, formats.weight_stats), with the spreads below given to the tensors its init leaves
# constant -- BatchNorm weights 1, biases 0, running means 0, running variances 1 and the zero-initialised Linear biases -- so that every
# BatchNorm fold and bias sum is exercised.  The reference module is then evaluated on the drawn weights (loaded with strict=True).
# Its 2-d blocks are torchvision's InvertedResidual: here the refshim stand-in written from the published block.
BOT_SPREAD = {'bn_weight': (1.0, 0.2), 'bn_bias': (0.0, 0.1), 'bn_running_mean': (0.0, 0.1), 'bn_log_running_var': (0.0, 0.3), 'bias': (0.0, 0.05)}


def _botanik_stats(sd, version):
    from azg_amd import formats
    out = formats.weight_stats(sd, seed=version)
    bn = {k.rsplit('.', 1)[0] for k in sd if k.endswith('running_var')}
    for k in sd:
        if 'shape/' + k not in out or '.' not in k:        # integer counters; the lowvalue buffer
            continue
        mod, leaf = k.rsplit('.', 1)
        if mod in bn:
            out['stat/' + k] = np.array(BOT_SPREAD['bn_log_running_var' if leaf == 'running_var' else 'bn_' + leaf])
        elif leaf == 'bias':
            out['stat/' + k] = np.array(BOT_SPREAD['bias'])
    out['arg/nn_version'] = np.array(version)
    return out


def botanik(version, n_vec=128, n_rand=16):
    """weightstats_botanik_v<version>.npz, netfwd_ (f32), netfwd64_ (f64) and netfwdrand_ (random int8 boards, all-valid masks, f32 and
    f64) from the reference's BotanikNNet on the stand-in weights"""
    import importlib
    import torch
    sys.path.insert(0, os.path.join(HERE, '..'))
    from azg_amd import formats
    m = H.load_reference()
    BN = importlib.import_module('botanik.BotanikNNet')
    g = m['BotanikGame'].BotanikGame()
    torch.manual_seed(version)
    model = BN.BotanikNNet(g, dict(nn_version=version, dropout=0.3)).eval()
    tag = 'botanik_v%d' % version
    stats = _botanik_stats({k: v.numpy() for k, v in model.state_dict().items()}, version)
    np.savez_compressed(os.path.join(GOLDEN, 'weightstats_%s.npz' % tag), **stats)
    sd = formats.synthetic_state_dict(np.load(os.path.join(GOLDEN, 'weightstats_%s.npz' % tag)))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    env = np.load(os.path.join(GOLDEN, 'env_botanik.npz'))
    sel = np.random.default_rng(0).choice(len(env['canonical']), size=min(n_vec, len(env['canonical'])), replace=False)
    shape, A = tuple(g.getBoardSize()), g.getActionSize()
    boards = env['canonical'][sel].reshape((-1,) + shape)
    masks = np.array([g.getValidMoves(b, 0) for b in boards]).astype(np.uint8)
    rboards = np.random.default_rng(1).integers(-128, 128, size=(n_rand,) + shape).astype(np.int8)
    rmasks = np.ones((n_rand, A), dtype=np.uint8)
    with torch.no_grad():
        out = [model(torch.from_numpy(b.astype(np.float32)), torch.from_numpy(k.astype(bool))) for b, k in ((boards, masks), (rboards, rmasks))]
        model = model.double()
        out64 = [model(torch.from_numpy(b.astype(np.float64)), torch.from_numpy(k.astype(bool))) for b, k in ((boards, masks), (rboards, rmasks))]
    (lp, v), (rlp, rv) = out
    (lp64, v64), (rlp64, rv64) = out64
    np.savez_compressed(os.path.join(GOLDEN, 'netfwd_%s.npz' % tag), boards=boards.astype(np.int8), masks=masks, pi=torch.exp(lp).numpy(),
                        v=v.numpy())
    np.savez_compressed(os.path.join(GOLDEN, 'netfwd64_%s.npz' % tag), pi64=torch.exp(lp64).numpy(), v64=v64.numpy())
    np.savez_compressed(os.path.join(GOLDEN, 'netfwdrand_%s.npz' % tag), boards=rboards, masks=rmasks, pi=torch.exp(rlp).numpy(),
                        v=rv.numpy(), pi64=torch.exp(rlp64).numpy(), v64=rv64.numpy())
    for name, a, b in (('game', (torch.exp(lp), v), (torch.exp(lp64), v64)), ('random', (torch.exp(rlp), rv), (torch.exp(rlp64), rv64))):
        print('%-12s %-6s boards |ref_f32 - ref_f64|: pi %.3g  v %.3g' % (tag, name, (a[0].double() - b[0]).abs().max(),
                                                                          (a[1].double() - b[1]).abs().max()))
    H.cleanup()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--f64':
        # `--f64` rewrites every netfwd64_*.npz; `--f64 TAG...` only those of the tags given
        for name, ckpt_rel, load_kw in F64:
            if len(sys.argv) == 2 or name in sys.argv[2:]:
                forward_f64(name, ckpt_rel, load_kw)
        return
    if len(sys.argv) > 2 and sys.argv[1] == '--random':
        # `--random TAG...`: netfwdrand_<tag>.npz, random int8 boards with all-valid masks through the reference module (f32 and f64)
        for name, ckpt_rel, load_kw in F64:
            if name in sys.argv[2:]:
                forward_random(name, ckpt_rel, load_kw)
        return
    if len(sys.argv) > 1 and sys.argv[1] == '--botanik':
        # `--botanik`: the stand-in fixtures of both Botanik versions (no checkpoint: see BOT_SPREAD)
        for version in (10, 11):
            botanik(version)
        return
    if len(sys.argv) > 2 and sys.argv[1] == '--only':
        return convert(*{'santorini11_v78': ('santorini11_v78', 'santorini/pretrained_withgods.pt', dict(santorini_gods=11),
                                             'SantoriniGame', 'SantoriniGame', 128),
                         # the two f4 games whose shipped checkpoints are nets of the MobileNet-1d family (MinivillesNNet.py:101-123
                         # nn_version 82, TLPNNet.py:175-196 nn_version 83): engine nets through nn_mb1d.hip.h
                         'minivilles2_v82': ('minivilles2_v82', 'minivilles/pretrained_2players.pt', dict(minivilles_players=2),
                                             'MinivillesGame', 'MinivillesGame', 128),
                         'tlp3_v83': ('tlp3_v83', 'thelittleprince/pretrained_3players.pt', dict(tlp_players=3), 'TLPGame', 'TLPGame', 128),
                         # the other shipped checkpoints of the family (every player count): the same kernel at their own geometries
                         'splendor3_v80': ('splendor3_v80', 'splendor/pretrained_3players.pt', dict(splendor_players=3), 'SplendorGame',
                                           'SplendorGame', 128),
                         'minivilles3_v82': ('minivilles3_v82', 'minivilles/pretrained_3players.pt', dict(minivilles_players=3),
                                             'MinivillesGame', 'MinivillesGame', 128),
                         'minivilles4_v82': ('minivilles4_v82', 'minivilles/pretrained_4players.pt', dict(minivilles_players=4),
                                             'MinivillesGame', 'MinivillesGame', 128),
                         'tlp4_v83': ('tlp4_v83', 'thelittleprince/pretrained_4players.pt', dict(tlp_players=4), 'TLPGame', 'TLPGame', 128),
                         'tlp5_v83': ('tlp5_v83', 'thelittleprince/pretrained_5players.pt', dict(tlp_players=5), 'TLPGame', 'TLPGame', 128),
                         # AbaloneNNet.py nn_version 21 (Belgian Daisy, the layout the engine plays): a 2-d MobileNet on the 9 x 9 grid,
                         # torchvision InvertedResidual blocks (the refshim stand-in); engine net through nn_abalone.hip.h
                         'abalone_v21': ('abalone_v21', 'abalone/pretrained_BelgianDaisy.pt', dict(), 'AbaloneGame', 'AbaloneGame', 128),
                         # the checkpoints of the two other layouts (the classic one from a dynamic-komi run): same net, same kernel
                         'abalone_v21_german': ('abalone_v21_german', 'abalone/pretrained_GermanDaisy.pt', dict(abalone_layout=2),
                                                'AbaloneGame', 'AbaloneGame', 128),
                         'abalone_v21_classic': ('abalone_v21_classic', 'abalone/pretrained_classic.pt',
                                                 dict(abalone_layout=0, abalone_dynamic_komi=True), 'AbaloneGame', 'AbaloneGame', 128),
                         # SmallworldNNet.py nn_version 62 (all three shipped checkpoints): a 3-layer transformer encoder over the
                         # (N, 8) tokens; engine net through nn_smallworld.hip.h
                         'smallworld_v62': ('smallworld_v62', 'smallworld/pretrained_2pl.pt', dict(smallworld_players=2), 'SmallworldGame',
                                            'SmallworldGame', 128),
                         'smallworld3_v62': ('smallworld3_v62', 'smallworld/pretrained_3pl.pt', dict(smallworld_players=3), 'SmallworldGame',
                                             'SmallworldGame', 128),
                         'smallworld4_v62': ('smallworld4_v62', 'smallworld/pretrained_4pl.pt', dict(smallworld_players=4), 'SmallworldGame',
                                             'SmallworldGame', 128),
                         # AkropolisNNet.py nn_version 31 (all three shipped checkpoints): board convolutions per player, a kernel-1
                         # InvertedResidual over the cells and a bilinear policy per construction-site tile; engine net through
                         # nn_akropolis.hip.h
                         'akropolis_v31': ('akropolis_v31', 'akropolis/pretrained_2pl.pt', dict(akropolis_players=2), 'AkropolisGame',
                                           'AkropolisGame', 128),
                         'akropolis3_v31': ('akropolis3_v31', 'akropolis/pretrained_3pl.pt', dict(akropolis_players=3), 'AkropolisGame',
                                            'AkropolisGame', 128),
                         'akropolis4_v31': ('akropolis4_v31', 'akropolis/pretrained_4pl.pt', dict(akropolis_players=4), 'AkropolisGame',
                                            'AkropolisGame', 128)}[sys.argv[2]])
    convert('splendor2_v80', 'splendor/pretrained_2players.pt', dict(splendor_players=2), 'SplendorGame', 'SplendorGame')
    convert('splendor4_v80', 'splendor/pretrained_4players.pt', dict(splendor_players=4), 'SplendorGame', 'SplendorGame', n_vec=128)
    convert('santorini1_v89', 'santorini/pretrained.pt', dict(santorini_gods=1), 'SantoriniGame', 'SantoriniGame', n_vec=128)
    convert('azul_v84', 'azul/pretrained.pt', dict(), 'AzulGame', 'AzulGame', n_vec=128)
    # V78 is built from torchvision.models.mobilenetv3.InvertedResidual.  torchvision is not installed here; tools/refshim
    # carries a functional stand-in written from the published block algorithm, so the reference's OWN SantoriniNNet.forward
    # (SantoriniNNet.py:264-271: gods embedding, heads, masking) runs on the unpickled full_model: the block body is pinned to
    # the published algorithm, everything around it to the reference
    convert('santorini11_v78', 'santorini/pretrained_withgods.pt', dict(santorini_gods=11), 'SantoriniGame', 'SantoriniGame',
            n_vec=128)


if __name__ == '__main__':
    main()
