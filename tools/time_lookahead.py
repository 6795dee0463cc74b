#!/usr/bin/env python
"""Device time of the one-ply lookahead (azg_env_lookahead, csrc/lookahead.hip.h) on the GPU, for Splendor-2p, Santorini without gods and
Abalone:

  1. the one launch on n positions against the loop of existing launches it replaces: for every action id that is valid in any of the
     positions, azg_env_next_state with that action on all n rows (rows where it is not valid step their first valid move: the loop has no
     way to skip them) and azg_env_game_ended on the result -- the same code as on the parent commit;
  2. the sweep over waves_per_state, at n positions and at 64 (an arena wave), which the host default (games.default_waves_per_state) rests on;
  3. a greedy ply -- lookahead_batch (with its four fills), greedy_candidates, pick_actions -- against a RandomContestant ply --
     valid_moves_batch, pick_actions;
  4. for orientation only: arena.vs_greedy of the shipped Splendor-2p and Abalone nets, 64 games, wall time.

The positions are canonical boards reached by random playouts of 2 .. 38 plies from fresh games (tools/time_history.py's recipe).  Every
figure is device time between two events around `--calls` back-to-back calls, after a warm-up call, the median of `--repeat` such runs
(all runs are printed); the loop of item 1 is timed whole, once per run.

    python tools/time_lookahead.py [--positions 4096] [--repeat 3] [--calls 10] [--games 64] [--sims 32] [--out FILE.md]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
SWEEP = (1, 2, 3, 4, 6, 8, 12, 16, 32, 64)


class Args(dict):
    __getattr__ = dict.get


def positions(g, n):
    caps = list(range(2, 40, 4))
    per = -(-n // len(caps))
    boards = []
    for j, cap in enumerate(caps):
        b0 = g.init_boards_batch(per, stream0=1000 * j)
        po = g.playouts_batch(b0, k=1, max_plies=cap, stream0=(1 << 20) * (j + 1), final_boards=True)
        live = po.status[:, 0] == 1                                   # (stopped at the cap: the game goes on and there is a move)
        boards.append(g.canonical_batch(po.boards[:, 0].contiguous(), po.players[:, 0].contiguous())[live])
    boards = torch.cat(boards)
    assert boards.shape[0] >= n // 2, 'too few open positions'
    return boards[torch.arange(n, device=boards.device) % boards.shape[0]].contiguous()


def device_us(fn, calls, repeat):
    """[microseconds per call] of `repeat` runs of `calls` back-to-back calls, after one warm-up call"""
    fn()
    out = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return out


def raw_lookahead(g, boards, bufs, w):
    from azg_amd._lib import check, lib
    from azg_amd.games import _ptr, _stream
    check(lib().azg_env_lookahead(g.GAME_ID, g.variant, _ptr(boards), None, None, boards.shape[0], w, C.c_uint64(g.rng_seed), C.c_uint64(0), None,
                                  _ptr(bufs.valid), _ptr(bufs.scores), _ptr(bufs.ended), _ptr(bufs.next_player), None, _stream()))


def measure(name, g, n, repeat, calls):
    from azg_amd.arena import PICK_UNIFORM, pick_actions
    from azg_amd.games import default_waves_per_state, greedy_candidates
    dev = g.device
    boards = positions(g, n)
    bufs = g.lookahead_batch(boards)
    valid = bufs.valid.bool()
    ids = valid.any(dim=0).nonzero()[:, 0].tolist()
    first = valid.int().argmax(dim=1).to(torch.int32)
    zero = torch.zeros(n, dtype=torch.int64, device=dev)
    rule = 'reference' if name != 'Santorini no gods' else 'lead'

    def loop():
        for a in ids:
            acts = torch.where(valid[:, a], torch.full_like(first, a), first)
            ns, npl = g.next_state_batch(boards, None, acts, zero)
            g.game_ended_batch(ns, npl)

    # the loop gives what the launch gives (scores of the valid rows), before anything is timed
    a0 = ids[len(ids) // 2]
    ns, npl = g.next_state_batch(boards, None, torch.where(valid[:, a0], torch.full_like(first, a0), first), zero)
    sc = g.game_ended_batch(ns, npl)[1]
    assert torch.equal(sc[valid[:, a0]], bufs.scores[:, a0][valid[:, a0]]), 'the launch and the loop disagree'
    w0 = default_waves_per_state(g.A)
    r = dict(game=name, positions=n, A=g.A, ids_valid_somewhere=len(ids), valid_per_position=float(valid.sum(dim=1).float().mean()),
             default_waves=w0)
    r['lookahead_us'] = device_us(lambda: raw_lookahead(g, boards, bufs, w0), calls, repeat)
    r['loop_us'] = device_us(loop, 1, repeat)
    r['sweep_us'] = {w: device_us(lambda: raw_lookahead(g, boards, bufs, w), calls, repeat) for w in SWEEP}
    few = boards[:64].contiguous()
    fbufs = g.lookahead_batch(few)
    r['sweep64_us'] = {w: device_us(lambda: raw_lookahead(g, few, fbufs, w), calls, repeat) for w in SWEEP}
    for key, b in (('ply', boards), ('ply64', few)):
        m = b.shape[0]
        counters = torch.zeros(m, dtype=torch.int64, device=dev)
        out = torch.zeros(m, dtype=torch.int32, device=dev)

        def greedy_ply():
            ahead = g.lookahead_batch(b)
            pick_actions(PICK_UNIFORM, None, greedy_candidates(g, rule, b, ahead.valid, ahead.scores), counters=counters, out=out)

        def random_ply():
            pick_actions(PICK_UNIFORM, None, g.valid_moves_batch(b, None), counters=counters, out=out)

        r[key + '_greedy_us'] = device_us(greedy_ply, calls, repeat)
        r[key + '_random_us'] = device_us(random_ply, calls, repeat)
    r['greedy_rule'] = rule
    return r


def strength(games_n, sims):
    """arena.vs_greedy of the shipped nets (orientation only)"""
    from azg_amd import games, nnet
    from azg_amd.arena import vs_greedy
    from tools_args import MCTS_ARGS
    G = os.path.join(ROOT, 'tests', 'golden')
    out = []
    for name, key, make_game, make_net in (
            ('Splendor-2p, V80', 'splendor2', lambda: games.SplendorGame(2),
             lambda: nnet.SplendorV80Hip.from_npz(os.path.join(G, 'weights_splendor2_v80.npz'), device='cuda:0', max_batch=games_n)),
            ('Abalone, V21', 'abalone', games.AbaloneGame,
             lambda: nnet.AbaloneV21Hip(nnet.AbaloneV21.from_npz(os.path.join(G, 'weights_abalone_v21.npz'), device='cuda:0'), max_batch=games_n))):
        try:
            g, net = make_game(), make_net()
            args = Args(numMCTSSims=sims, prob_fullMCTS=1.0, ratio_fullMCTS=5, dirichletAlpha=0, temperature=[1, 1, 1], **MCTS_ARGS[key])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            won, lost, draws = vs_greedy(g, net, args, games_n)
            torch.cuda.synchronize()
            out.append(dict(match=name, games=games_n, sims=sims, won=won, lost=lost, draws=draws, seconds=time.perf_counter() - t0))
        except Exception as e:                                          # orientation only: a net that does not load is reported, not fatal
            out.append(dict(match=name, error='%s: %s' % (type(e).__name__, e)))
        print(json.dumps(out[-1]), flush=True)
    return out


def med(xs):
    return statistics.median(xs)


def markdown(results, matches):
    fmt = lambda xs: ' / '.join('%.1f' % x for x in xs)  # noqa: E731
    out = ['| game | positions | A | ids valid somewhere | valid moves per position | one launch, default waves (µs), per run | the loop it replaces (µs), per run | loop / launch (medians) |',
           '|---|---|---|---|---|---|---|---|']
    for r in results:
        out.append('| %s | %d | %d | %d | %.1f | %s (waves_per_state %d) | %s | %.0f x |' % (
            r['game'], r['positions'], r['A'], r['ids_valid_somewhere'], r['valid_per_position'], fmt(r['lookahead_us']), r['default_waves'],
            fmt(r['loop_us']), med(r['loop_us']) / med(r['lookahead_us'])))
    for key, what in (('sweep_us', 'all positions'), ('sweep64_us', '64 positions')):
        out += ['', 'waves_per_state sweep, %s: median µs per launch' % what, '', '| game | ' + ' | '.join(str(w) for w in SWEEP) + ' |',
                '|---|' + '---|' * len(SWEEP)]
        for r in results:
            out.append('| %s | ' % r['game'] + ' | '.join('%.1f' % med(r[key][w]) for w in SWEEP) + ' |')
    out += ['', '| game | rule | greedy ply, all positions (µs), per run | random ply, all positions (µs), per run | greedy ply, 64 positions (µs), per run | random ply, 64 positions (µs), per run |',
            '|---|---|---|---|---|---|']
    for r in results:
        out.append('| %s | %s | %s | %s | %s | %s |' % (r['game'], r['greedy_rule'], fmt(r['ply_greedy_us']), fmt(r['ply_random_us']),
                                                       fmt(r['ply64_greedy_us']), fmt(r['ply64_random_us'])))
    if matches:
        out += ['', 'vs_greedy (orientation only): won / lost / draws from the net\'s side', '']
        for m in matches:
            out.append('    %-20s %s' % (m['match'], m.get('error') or '%d / %d / %d   (%d games, numMCTSSims %d, %.1f s)' % (
                m['won'], m['lost'], m['draws'], m['games'], m['sims'], m['seconds'])))
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--positions', type=int, default=4096)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--games', type=int, default=64, help='games of the vs_greedy matches; 0: none')
    ap.add_argument('--sims', type=int, default=32, help='numMCTSSims of the nets in the vs_greedy matches')
    ap.add_argument('--out', default=None, help='write the markdown tables and the JSON lines here as well')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_lookahead.py measures on the GPU: no device found')
    from azg_amd import games
    results = []
    for name, make in (('Splendor-2p', lambda: games.SplendorGame(2)), ('Santorini no gods', lambda: games.SantoriniGame(1)),
                       ('Abalone', games.AbaloneGame)):
        results.append(measure(name, make(), a.positions, a.repeat, a.calls))
        print(json.dumps(results[-1]), flush=True)
        torch.cuda.empty_cache()
    matches = strength(a.games, a.sims) if a.games > 0 else []
    text = markdown(results, matches)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n\n' + '\n'.join(json.dumps(r) for r in results + matches) + '\n')


if __name__ == '__main__':
    main()
