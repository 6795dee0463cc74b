#!/usr/bin/env python3
"""Time one training step of train.train on the GPU in one process: the legacy path, device_batches=True, the eager device optimiser
(device_optimizer=True) and a step as one graph replay (graph_step=True).
    python tools/time_train_step.py [--out profiles/r14_train_graph_step.md] [--sizes 65536,1048576] [--batch 512] [--warmup 50] [--steps 200]
The Splendor-2p SplendorV80Module on n synthetic examples.  Per n and per path train.train itself runs warmup + steps optimiser steps
(stopped from its on_step hook); the clock runs from a device synchronise after the warm-up to one after the last timed step, so the
figure is wall time per step with everything a path makes the host do.  The paths alternate, `--repeats` rounds per size.  Separately: the
kernel time of the batch launches by device events (sample_ids for one epoch of n // batch steps; gather and losses for one batch), of the
optimiser's two launches on the V80 parameter set against torch's AdamW step on the same set, and the CPU time of one torch.randperm(n),
which the legacy path pays per step.  Prints a markdown report (and writes it to --out).
    python tools/time_train_step.py --compact [--compact-records 32768] [--batch 512] [--repeats 2] [--out FILE.md]
The graph_step path alone on one Splendor-2p history (the synthetic records of tools/time_history.py), read as expanded rows
(history.DeviceHistory.columns(), the path before the compact history) and as records (history.CompactHistory), alternating; with the
kernel time of the two gathers on the same batch (20 launches captured in one graph, replayed)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Stop(Exception):
    pass


def synthetic(n, device, seed=0):
    """five columns on the device: int8 boards [n, 392], normalised pi on random valid sets [n, 81], z = +-1 per seat, valids u8, q"""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    boards = torch.randint(0, 8, (n, 392), generator=g, device=device, dtype=torch.int8)
    valids = torch.rand((n, 81), generator=g, device=device) < 0.4
    valids[:, 0] = True
    pi = torch.rand((n, 81), generator=g, device=device) * valids
    pi = pi / pi.sum(1, keepdim=True)
    z = torch.where(torch.rand((n, 1), generator=g, device=device) < 0.5, 1.0, -1.0) * torch.tensor([[1.0, -1.0]], device=device)
    q = 0.5 * z * torch.rand((n, 2), generator=g, device=device)
    return boards, pi.float(), z.float(), valids.to(torch.uint8), q.float()


PATHS = (('legacy', dict()), ('device_batches', dict(device_batches=True)),
         ('device_optimizer', dict(device_batches=True, device_optimizer=True)), ('graph_step', dict(device_batches=True, graph_step=True)))


def time_path(ex, batch, warmup, steps, switches):
    import torch
    from azg_amd import train
    n = ex.n if hasattr(ex, 'n_records') else ex[0].shape[0]
    spe = n // batch
    epochs = -(-(warmup + steps) // spe)
    mark = {}

    def on_step(ep, i_batch, step):
        if step + 1 == warmup:
            torch.cuda.synchronize()
            mark['t0'] = time.perf_counter()
        elif step + 1 == warmup + steps:
            torch.cuda.synchronize()
            mark['t1'] = time.perf_counter()
            raise _Stop

    torch.manual_seed(0)
    m = train.SplendorV80Module(num_players=2, dropout=0.0)
    try:
        train.train(m, ex, learn_rate=3e-4, batch_size=batch, epochs=epochs, q_weight=0.5, device='cuda:0', seed=1, on_step=on_step,
                    **switches)
    except _Stop:
        pass
    return (mark['t1'] - mark['t0']) / steps * 1e3


def event_ms(fn, reps=200, warm=20):
    import torch
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def compact_report(args):
    """--compact: graph_step on expanded rows against graph_step on records, one history"""
    import statistics
    import torch
    from azg_amd import games, train
    from azg_amd.history import CompactHistory, DeviceHistory
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from time_history import graph_us, synthetic_records
    g = games.SplendorGame(2)
    recs = synthetic_records(g, args.compact_records)
    d, c = DeviceHistory(g.S, g.A, g.P, device=g.device), CompactHistory(g.S, g.A, g.P, device=g.device)
    assert d.append_records(g, recs, stream0=1 << 42) == c.append_records(g, recs, stream0=1 << 42)
    cols = d.columns()
    runs = {'expanded': [], 'compact': []}
    for _ in range(args.repeats):
        runs['expanded'].append(time_path(cols, args.batch, args.warmup, args.steps, dict(device_batches=True, graph_step=True)))
        runs['compact'].append(time_path(c, args.batch, args.warmup, args.steps, dict(device_batches=True, graph_step=True)))
    ids = torch.randint(0, d.n, (args.batch,), generator=torch.Generator(device='cpu').manual_seed(3)).to(torch.int32).to(g.device)
    outs = train.gather_batch(cols, ids)
    k_exp, k_cmp = [], []
    for _ in range(2):
        k_exp.append(graph_us(lambda: train.gather_batch(cols, ids, out=outs)))
        k_cmp.append(graph_us(lambda: c.gather(ids, out=outs)))
    dk = (statistics.median(k_cmp) - statistics.median(k_exp)) / 1e3
    spread = max(runs['expanded']) - min(runs['expanded'])
    fmt = lambda xs, f='%.3f': ' / '.join(f % x for x in xs)  # noqa: E731
    bound = statistics.median(runs['expanded']) + max(dk, 0.0) + spread
    lines = ['# `graph_step` on a compact history against the expanded rows (`tools/time_train_step.py --compact`)', '',
             '%s, torch %s.  SplendorV80Module (2 players), batch %d, %d warm-up + %d timed steps per run, alternating in one process.'
             % (torch.cuda.get_device_name(0), torch.__version__, args.batch, args.warmup, args.steps),
             'Splendor-2p: %d records, %d rows; %.1f MiB as expanded rows, %.1f MiB as records.'
             % (c.n_records, c.n, d.n * c.row_bytes / 2 ** 20, c.device_bytes() / 2 ** 20), '',
             '| | expanded rows | compact |', '|---|---|---|',
             '| `graph_step` step (ms), per run | %s | %s |' % (fmt(runs['expanded']), fmt(runs['compact'])),
             '| gather kernel, B = %d (µs), per run | %s | %s |' % (args.batch, fmt(k_exp, '%.1f'), fmt(k_cmp, '%.1f')), '',
             'd (kernel-time difference of the medians) = %.4f ms, s (spread of the expanded runs) = %.4f ms: the compact step is accepted up to'
             % (dk, spread),
             'median(expanded) + d + s = %.4f ms; its median is %.4f ms -- %s.'
             % (bound, statistics.median(runs['compact']), 'within' if statistics.median(runs['compact']) <= bound else 'ABOVE the bound')]
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--out', default=None)
    ap.add_argument('--sizes', default='65536,1048576')
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=2, help='alternating rounds of the four paths per size')
    ap.add_argument('--compact', action='store_true', help='graph_step on a CompactHistory against the expanded rows (see above)')
    ap.add_argument('--compact-records', type=int, default=32768, help='Splendor-2p records of the --compact history')
    args = ap.parse_args(argv)
    import torch
    from azg_amd import train
    if not torch.cuda.is_available():
        raise SystemExit('time_train_step: needs a GPU (a CPU timing says nothing about it)')
    if args.compact:
        return compact_report(args)
    dev = 'cuda:0'
    lines = ['# Training step: legacy, `device_batches`, `device_optimizer`, `graph_step` (`tools/time_train_step.py`)', '',
             '%s, torch %s.  SplendorV80Module (2 players), batch %d, %d warm-up + %d timed optimiser steps per run, the four paths in one'
             % (torch.cuda.get_device_name(0), torch.__version__, args.batch, args.warmup, args.steps),
             'process, alternating; wall time between two device synchronisations / steps.  The legacy path is `train.train` with its defaults;',
             '`device_optimizer` and `graph_step` run with `device_batches=True`.', '',
             '| n examples | legacy step (ms), per run | `device_batches` step (ms), per run | eager `device_optimizer` step (ms), per run | `graph_step` step (ms), per run | `device_optimizer` / `device_batches` (best of each) | `graph_step` / `device_batches` (best of each) | one `torch.randperm(n)` on the CPU (ms) |',
             '|---|---|---|---|---|---|---|---|']
    kern = ['', '## Kernel time of the batch launches (device events, mean of 200 calls; 50 for the draw)', '',
            '| n examples | `azg_train_sample_ids`, one epoch = n // batch steps (µs) | per step of that epoch (µs) | `azg_train_gather`, one batch (µs) | `azg_train_losses`, both launches (µs) |',
            '|---|---|---|---|---|']
    for n in [int(x) for x in args.sizes.split(',')]:
        ex = synthetic(n, dev)
        runs = {name: [] for name, _ in PATHS}
        for _ in range(args.repeats):
            for name, switches in PATHS:
                runs[name].append(time_path(ex, args.batch, args.warmup, args.steps, switches))
        g = torch.Generator(device='cpu')
        g.manual_seed(1)
        torch.randperm(n, generator=g)
        t0 = time.perf_counter()
        for _ in range(10):
            torch.randperm(n, generator=g)
        perm_ms = (time.perf_counter() - t0) / 10 * 1e3
        fmt = lambda xs: ' / '.join('%.3f' % x for x in xs)  # noqa: E731
        best = {name: min(xs) for name, xs in runs.items()}
        lines.append('| %d | %s | %s | %s | %s | %.3f | %.3f | %.3f |' % (
            n, fmt(runs['legacy']), fmt(runs['device_batches']), fmt(runs['device_optimizer']), fmt(runs['graph_step']),
            best['device_optimizer'] / best['device_batches'], best['graph_step'] / best['device_batches'], perm_ms))
        # the three launches on their own
        spe = n // args.batch
        ids = torch.empty((spe, args.batch), dtype=torch.int32, device=dev)
        t_ids = event_ms(lambda: train.sample_ids(n, args.batch, spe, 1, 0, out=ids), reps=50, warm=5)
        cols = tuple(x.contiguous() for x in (ex[0], ex[1], ex[2], ex[3], ex[4]))
        outs = train.gather_batch(cols, ids[0])
        t_gather = event_ms(lambda: train.gather_batch(cols, ids[0], out=outs))
        lp = torch.log_softmax(torch.randn((args.batch, 81), device=dev), 1)
        v = torch.tanh(torch.randn((args.batch, 2), device=dev))
        out2 = torch.empty(2, dtype=torch.float64, device=dev)
        t_loss = event_ms(lambda: train.train_losses(lp, v, outs[1], outs[2], outs[4], 0.5, out=out2))
        kern.append('| %d | %.1f | %.3f | %.1f | %.1f |' % (n, t_ids * 1e3, t_ids * 1e3 / spe, t_gather * 1e3, t_loss * 1e3))
        del ex, cols, outs
        torch.cuda.empty_cache()
    kern += ['', '(The device path draws an epoch\'s ids with one launch before the epoch\'s first step: where an epoch is longer than the warm-up',
             'that launch is outside the timed window, and its share of a step is the third column.)',
             '', '(The event figures include the Python wrapper\'s argument checks and, for the losses, its three buffer allocations between the',
             'launches: they are the cost of the call as the trainer makes it, an upper bound of the kernels\' own time.)']
    # the optimiser on the V80 parameter set: the two new launches against torch's own AdamW step (its foreach launches, host included)
    m = train.SplendorV80Module(num_players=2, dropout=0.0).to(dev)
    params = [p for p in m.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    ref = torch.optim.AdamW(params, lr=3e-4)
    t_ref = event_ms(ref.step)
    grads = [p.grad.clone() for p in params]
    mine = train.DeviceAdamW(params, 3e-4, 1000)
    for p, gr in zip(params, grads):
        p.grad = gr
    mine.step()                                                          # the first step moves the gradients into the flat buffer

    def both():
        train.adamw_update(mine.segs, mine.chunks, mine.table, mine.step_counter)
        train.adamw_step_advance(mine.step_counter)

    t_both = event_ms(both)
    t_upd = event_ms(lambda: train.adamw_update(mine.segs, mine.chunks, mine.table, mine.step_counter))
    kern += ['', '## The optimiser step on the V80 parameter set (device events, mean of 200 calls)', '',
             '%d parameter tensors, %d floats, %d workgroups of 2048 elements.' % (len(params), sum(p.numel() for p in params), mine.chunks.shape[0]), '',
             '| `azg_train_adamw` alone (µs) | `azg_train_adamw` + `azg_train_step_advance` (µs) | `torch.optim.AdamW.step()`, foreach (µs) |', '|---|---|---|',
             '| %.1f | %.1f | %.1f |' % (t_upd * 1e3, t_both * 1e3, t_ref * 1e3),
             '', '(Back-to-back calls from Python: where the host issues slower than the GPU runs, the figure is the host\'s issue time per call,',
             'an upper bound of the kernels\' own time.)']
    text = '\n'.join(lines + kern) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
