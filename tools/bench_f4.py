"""Throughput of the six f4 game plugins on one MI355X ("each to the same parity + measurement bar"): batched
self-play on the engine with the integer hash-net of SURVEY Appendix C.3 as the leaf evaluator (these games have no engine net; the
figure is the env step + tree side of the plugin, `nnet.TorchModuleEvaluator` adds the user's PyTorch-ROCm module on top).
    python tools/bench_f4.py [--games 1024 --sims 200 --plies 12]
    python tools/bench_f4.py --net engine --pipe --only smallworld    (the V62 net on the asynchronous tree pipeline, csrc/azg_async.hip.h)
    python tools/bench_f4.py --net engine --pipe --only minivilles    (... and the V82 / V83 MobileNet-1d nets of Minivilles / TLP)
One JSON line per game: plies/s, simulations/s, ms per round, levels per simulation, valid actions per level, engine errors,
structural validation of the forest afterwards."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from azg_amd import games  # noqa: E402
from azg_amd.selfplay import SelfPlayEngine  # noqa: E402
from hashnet import HashNetHip, HashNetTorch  # noqa: E402


class Args(dict):
    __getattr__ = dict.get


# (name, constructor, share of --games, node capacity in units of numMCTSSims: a Smallworld round spans both players' whole turns, so
#  the round-based clean-up keeps ~30 plies of nodes)
GAMES = [('minivilles', lambda: games.MinivillesGame(2), 1.0, 10), ('abalone', games.AbaloneGame, 1.0, 10), ('thelittleprince', lambda: games.TLPGame(3), 1.0, 10),
         ('botanik', games.BotanikGame, 1.0, 10), ('akropolis', games.AkropolisGame, 0.25, 10), ('smallworld', lambda: games.SmallworldGame(2), 1.0, 80),
         ('smallworld3', lambda: games.SmallworldGame(3), 0.5, 80), ('smallworld4', lambda: games.SmallworldGame(4), 0.5, 80),
         ('akropolis3', lambda: games.AkropolisGame(3), 0.25, 10), ('akropolis4', lambda: games.AkropolisGame(4), 0.25, 10),
         ('minivilles3', lambda: games.MinivillesGame(3), 1.0, 10), ('minivilles4', lambda: games.MinivillesGame(4), 1.0, 10),
         ('tlp4', lambda: games.TLPGame(4), 1.0, 10), ('tlp5', lambda: games.TLPGame(5), 1.0, 10)]


class MlpNet(torch.nn.Module):
    """A PyTorch module with the reference's forward signature and the size of its small per-game nets (flatten -> 256 -> 256 -> 128 with
    LayerNorm + SiLU, two-layer policy and value heads: the shape of MinivillesNNet V83; the reference ships 2-8 architectures per game,
    they are not restated here).  Random weights: the figure is the cost of a real module per round through nnet.TorchModuleEvaluator."""

    def __init__(self, n_in, A, P):
        super().__init__()
        nn = torch.nn
        self.trunk = nn.Sequential(nn.Linear(n_in, 256), nn.LayerNorm(256), nn.SiLU(), nn.Linear(256, 256), nn.LayerNorm(256), nn.SiLU(),
                                   nn.Linear(256, 128), nn.LayerNorm(128), nn.SiLU())
        self.pi = nn.Sequential(nn.Linear(128, 64), nn.SiLU(), nn.Linear(64, A))
        self.v = nn.Sequential(nn.Linear(128, 64), nn.SiLU(), nn.Linear(64, P))

    def forward(self, x, valid):
        h = self.trunk(x.flatten(1))
        pi = torch.where(valid, self.pi(h), torch.full((), -1e8, device=x.device))
        return torch.log_softmax(pi, dim=1), torch.tanh(self.v(h))


# the rows whose engine nets have a kind in the asynchronous tree pipeline (opt-in there: async_pipe=True)
PIPE_ROWS = ('smallworld', 'smallworld3', 'smallworld4', 'minivilles', 'minivilles3', 'minivilles4', 'thelittleprince', 'tlp4', 'tlp5')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--net', default='hash', choices=['hash', 'hashhip', 'mlp', 'engine', 'torchnet'],
                    help='leaf evaluator: integer hash-net as torch ops, the same as one engine kernel (azg_eval_hashnet), MlpNet through TorchModuleEvaluator, '
                         'engine = the game\'s SHIPPED net (minivilles/pretrained_{2,3,4}players.pt V82, thelittleprince/pretrained_{3,4,5}players.pt V83: the engine\'s '
                         'MobileNet-1d kernel, nn_mb1d.hip.h; abalone/pretrained_BelgianDaisy.pt V21: nn_abalone.hip.h; smallworld/pretrained_{2,3,4}pl.pt '
                         'V62: nn_smallworld.hip.h; akropolis/pretrained_{2,3,4}pl.pt V31: nn_akropolis.hip.h; Botanik, which ships no checkpoint: the V10 stand-in '
                         'weights of weightstats_botanik_v10.npz through nn_botanik.hip.h) as one launch; torchnet = the same weights as '
                         'PyTorch-ROCm ops (nnet.MobileNet1d, nnet.AbaloneV21, nnet.SmallworldV62, nnet.AkropolisV31, nnet.BotanikV1x)')
    ap.add_argument('--md', action='store_true', help='markdown table row instead of JSON')
    ap.add_argument('--games', type=int, default=1024)
    ap.add_argument('--sims', type=int, default=200)
    ap.add_argument('--plies', type=int, default=40, help='timed ply waves (one wave = `sims` lock-step rounds)')
    ap.add_argument('--only', default=None, help='rows to run (comma-separated names)')
    ap.add_argument('--pipe', action='store_true', help='with --net engine: run the Smallworld, Minivilles and The Little Prince rows on the asynchronous '
                                                           'tree pipeline (async_pipe=True; AZG_ASYNC_NNET / AZG_ASYNC_NSEL set the CU split) and report its '
                                                           'profile; other rows are skipped')
    ap.add_argument('--cyc', action='store_true', help='cycle breakdown of k_select per tree and launch (a library built with AZG_DEFINES=AZG_CYC_COUNTERS)')
    a = ap.parse_args()
    for name, make, scale, capf in GAMES:
        if a.only and name not in a.only.split(','):
            continue
        pipe = a.pipe and a.net == 'engine'
        if pipe and name not in PIPE_ROWS:
            continue
        g = make()
        T = max(64, int(a.games * scale))
        # (Akropolis offers hundreds of placements: with 200 simulations policy-target pruning leaves no count above 1, error bit 64)
        args = Args(numMCTSSims=a.sims, cpuct=1.0, fpu=0.0, universes=1, forced_playouts=not name.startswith('akropolis'), prob_fullMCTS=1.0, ratio_fullMCTS=5,
                    dirichletAlpha=0.3, temperature=[1.25, 0.8, 1.0], tempThreshold=6)
        if a.net in ('engine', 'torchnet'):
            tag = {'minivilles': 'minivilles2_v82', 'thelittleprince': 'tlp3_v83', 'abalone': 'abalone_v21', 'smallworld': 'smallworld_v62',
                   'smallworld3': 'smallworld3_v62', 'smallworld4': 'smallworld4_v62', 'akropolis': 'akropolis_v31', 'akropolis3': 'akropolis3_v31',
                   'akropolis4': 'akropolis4_v31', 'minivilles3': 'minivilles3_v82', 'minivilles4': 'minivilles4_v82', 'tlp4': 'tlp4_v83',
                   'tlp5': 'tlp5_v83', 'botanik': 'botanik_v10'}.get(name)
            if tag is None:
                continue
            from azg_amd import nnet
            w = os.path.join(ROOT, 'tests', 'golden', 'weights_%s.npz' % tag)
            if name == 'abalone':           # abalone/pretrained_BelgianDaisy.pt V21: the engine's one-launch kernel (nn_abalone.hip.h)
                base = nnet.AbaloneV21.from_npz(w, device='cuda:0')
                net = nnet.AbaloneV21Hip(base, max_batch=T) if a.net == 'engine' else base
            elif name.startswith('smallworld'):     # smallworld/pretrained_{2,3,4}pl.pt V62: the one-launch transformer kernel (nn_smallworld.hip.h)
                base = nnet.SmallworldV62.from_npz(w, num_players=g.P, device='cuda:0')
                net = nnet.SmallworldV62Hip(base, max_batch=T) if a.net == 'engine' else base
            elif name.startswith('akropolis'):      # akropolis/pretrained_{2,3,4}pl.pt V31: the one-launch kernel (nn_akropolis.hip.h)
                base = nnet.AkropolisV31.from_npz(w, num_players=g.P, device='cuda:0')
                net = nnet.AkropolisV31Hip(base, max_batch=T) if a.net == 'engine' else base
            elif name == 'botanik':         # no checkpoint: the V10 stand-in weights, the one-launch kernel (nn_botanik.hip.h)
                from azg_amd import formats
                base = nnet.BotanikV1x(formats.fixture_state_dict(os.path.join(ROOT, 'tests', 'golden'), tag)[0], device='cuda:0')
                net = nnet.BotanikV1xHip(base, max_batch=T) if a.net == 'engine' else base
            else:                           # (Minivilles 4p: the stand-in weights of the same shapes, weightstats_minivilles4_v82.npz)
                from azg_amd import formats
                base = nnet.MobileNet1d(formats.fixture_state_dict(os.path.join(ROOT, 'tests', 'golden'), tag)[0], device='cuda:0')
                net = nnet.MobileNet1dHip(base, max_batch=T) if a.net == 'engine' else base
        elif a.net == 'mlp':
            from azg_amd.nnet import TorchModuleEvaluator
            torch.manual_seed(0)
            net = TorchModuleEvaluator(MlpNet(int(g.S), g.A, g.P), g)
        elif a.net == 'hashhip':
            net = HashNetHip(g.P)
            net.bind_outputs(T, g.A, g.P, g.device)          # fixed output buffers: the engine's expansion reads them in place (no copy kernels per round)
        else:
            net = HashNetTorch(g.P)
        eng = SelfPlayEngine(g, net, args, n_games=T, node_capacity=max(2048, capf * a.sims), max_examples=T * 256, **(dict(async_pipe=True) if pipe else {}))
        eng.start()
        eng.run(2 * a.sims)                                    # warm-up: two ply waves (also captures the HIP graph)
        torch.cuda.synchronize()
        if pipe:
            eng.forest.async_profile(reset=True)
        s0 = eng.stats()
        t0 = time.perf_counter()
        eng.run(a.plies * a.sims)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        s1 = eng.stats()
        sims, plies = s1['sims'] - s0['sims'], s1['plies'] - s0['plies']
        prof = eng.forest.async_profile(reset=True) if pipe else None
        bad = sum(grp.f.validate(verbose=False) for grp in eng.groups)
        evaluator = a.net + ('+pipe' if pipe else '')
        if a.md:
            print('| %s | %d | %d | %d | %d | %s | %.0f | %.2f | %.3f | %.2f | %.1f | %d | %d | %.1f |' % (
                name, g.P, g.S, g.A, T, evaluator, plies / dt, sims / dt / 1e6, dt / (a.plies * a.sims) * 1e3, (s1['levels'] - s0['levels']) / max(sims, 1),
                (s1['sum_valid_visited'] - s0['sum_valid_visited']) / max(s1['levels'] - s0['levels'], 1), s1['errors'], bad, eng.device_bytes / 1e9), flush=True)
        else:
            print(json.dumps(dict(game=name, players=g.P, state_bytes=g.S, actions=g.A, games=T, sims_per_move=a.sims, plies_per_s=plies / dt,
                                  sims_per_s=sims / dt, ms_per_round=dt / (a.plies * a.sims) * 1e3,
                                  levels_per_sim=(s1['levels'] - s0['levels']) / max(sims, 1),
                                  valid_per_level=(s1['sum_valid_visited'] - s0['sum_valid_visited']) / max(s1['levels'] - s0['levels'], 1),
                                  games_finished=s1['games'], errors=s1['errors'], validate_violations=bad,
                                  forest_gb=eng.device_bytes / 1e9, evaluator=evaluator,
                                  **({} if prof is None else dict(pipeline={k: prof[k] for k in ('n_sel', 'n_net', 'descent_us', 'forward_us', 'leaves_per_batch',
                                                                                                   'leaf_wait_us', 'ready_wait_us', 'select_wave_busy', 'net_wg_busy',
                                                                                                   'launches', 'timeouts')})))), flush=True)
        if a.cyc and 'cyc_seg' in s1:
            n = a.plies * a.sims * T
            seg = [s1['cyc_seg'][k] - s0['cyc_seg'][k] for k in range(4)]
            d = {k: s1[k] - s0[k] for k in ('cyc_select', 'cyc_levels', 'cyc_edge', 'cyc_leaf', 'levels', 'sims', 'expansions', 'terminal_hits')}
            print('  %s per tree-launch cycles: select %.0f = levels %.0f (%.2f levels, %.0f each) + edge %.0f (prologue+load_state %.0f make_move %.0f canon+hash %.0f probe %.0f) '
                  '+ leaf %.0f + rest %.0f; expansions %.3f terminal %.3f' % (
                      name, d['cyc_select'] / n, d['cyc_levels'] / n, d['levels'] / n, d['cyc_levels'] / max(1, d['levels']), d['cyc_edge'] / n, seg[0] / n, seg[1] / n, seg[2] / n,
                      seg[3] / n, d['cyc_leaf'] / n, (d['cyc_select'] - d['cyc_levels'] - d['cyc_edge'] - d['cyc_leaf']) / n, d['expansions'] / n, d['terminal_hits'] / n), flush=True)
        for grp in eng.groups:
            grp.f.close()
        del eng
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
