#!/usr/bin/env python
"""Wall time from "an iteration's records are drained" to "columns the trainer can read", on the GPU, for the two ways Coach.learn gets there:

  (a) the default path: Coach._collect (sort, symmetries_batch into [n, K, .], mask + repeat_interleave), formats.examples_to_iteration
      (device -> host, pickle + zlib per row), then what learn() and NNetWrapper.train do before the first step: concatenate the history of H
      iterations, shuffle, decode_examples (decompress + unpickle every row of every iteration, np.stack), upload;
  (b) the device history: DeviceHistory.append_records (azg_examples_expand: count pass, prefix sum, one host read, write pass) behind
      H - 1 iterations that are already there; columns() are views.  pop_oldest of a full history is timed on its own.

The records are synthetic but realistic: boards reached by random playouts of 2 .. 38 plies from fresh games, made canonical, with their
valid moves, a random policy on them and random z / q.  Both paths get the same records and the same symmetry streams, and their columns
are compared before anything is timed.  Each expansion's torch.cuda.max_memory_allocated above the records themselves is reported, the rows it produces included.

    python tools/time_history.py [--records-splendor 8192] [--records-azul 1024] [--history 5] [--repeat 3] [--out FILE.md]

Every timing ends in a device synchronise; (b) is the median of --repeat runs, (a) runs once (it is host loops over every row).

    python tools/time_history.py --compact [--records-splendor 32768] [--records-azul 4096] [--records-tlp 8192] [--batch 512] [--out FILE.md]

The compact history (history.CompactHistory) against the device history on the same records, alternating in one process: append_records
wall time (the compact one has no write pass), live device bytes (from the shapes, checked against device_bytes()), and the kernel time
of one batch -- azg_train_gather_forms on the records against azg_train_gather on the expanded rows, the same ids, each as 20 launches
captured in one graph and replayed (no host between the launches).  The rows of both are compared before anything is timed."""
import argparse
import json
import os
import random
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def synthetic_records(g, n, seed=5):
    """n records (boards, pi, z, valids, q, meta) on g.device"""
    dev = g.device
    caps = list(range(2, 40, 4))
    per = -(-n // len(caps))
    boards = []
    for j, cap in enumerate(caps):
        b0 = g.init_boards_batch(per, stream0=1000 * j)
        po = g.playouts_batch(b0, k=1, max_plies=cap, stream0=(1 << 20) * (j + 1), final_boards=True)
        boards.append(g.canonical_batch(po.boards[:, 0].contiguous(), po.players[:, 0].contiguous()))
    boards = torch.cat(boards)[:n].contiguous()
    valids = g.valid_moves_batch(boards, torch.zeros(n, dtype=torch.int32, device=dev))
    gen = torch.Generator(device='cpu').manual_seed(seed)
    pi = torch.rand((n, g.A), generator=gen).to(dev) * valids
    pi = (pi / pi.sum(1, keepdim=True).clamp_min(1e-9)).contiguous()
    z = torch.randn((n, g.P), generator=gen).to(dev)
    q = torch.randn((n, g.P), generator=gen).to(dev)
    i = torch.arange(n, dtype=torch.int32)
    meta = torch.stack([i % 64, (i // 64) % 7, i // 448, torch.zeros_like(i)], dim=1)      # (stream, game index, ply, -)
    meta = meta[torch.randperm(n, generator=gen)].to(dev).contiguous()                     # drained in no particular order
    return [boards, pi, z, valids, q, meta]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def peak_above(fn):
    """(seconds, result, peak of torch's allocated bytes above what was allocated before the call)"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    dt, out = timed(fn)
    return dt, out, torch.cuda.max_memory_allocated() - base


def default_path(g, recs, H, maxlen, stream_offset=0):
    """-> (dict of phase times, device columns of the H-iteration history, peak bytes of the expansion)"""
    from azg_amd import formats
    from azg_amd.coach import Coach
    from azg_amd.nnet_wrapper import decode_examples
    stub = types.SimpleNamespace(game=g, dist=None, _sym_stream=stream_offset)
    t_collect, ex, peak = peak_above(lambda: Coach._collect(stub, [tuple(recs)]))
    t_encode, it = timed(lambda: formats.examples_to_iteration(ex, tuple(g.getBoardSize()), compress=True, maxlen=maxlen))
    del ex

    def decode():
        examples = [e for h in [it] * H for e in h]
        random.Random(1).shuffle(examples)
        cols = decode_examples(examples)
        return [torch.as_tensor(c).to(g.device) for c in cols]

    t_decode, cols = timed(decode)
    return dict(collect=t_collect, encode=t_encode, decode_upload=t_decode, total=t_collect + t_encode + t_decode, rows=len(it)), cols, peak


def device_path(g, recs, H, maxlen, repeat, stream_offset=0):
    from azg_amd.history import DeviceHistory
    s0 = (1 << 42) + stream_offset
    probe = DeviceHistory(g.S, g.A, g.P, device=g.device)
    rows, _ = probe.append_records(g, recs, maxlen=maxlen, stream0=s0)
    first = [c.clone() for c in probe.columns()]
    del probe
    times, peaks = [], []
    for _ in range(repeat):
        h = DeviceHistory(g.S, g.A, g.P, device=g.device, capacity=(H + 1) * rows)
        for _ in range(H - 1):
            h.append_columns(first)
        dt, _, peak = peak_above(lambda: (h.append_records(g, recs, maxlen=maxlen, stream0=s0), h.columns()))
        times.append(dt)
        peaks.append(peak)
        t_pop, _ = timed(h.pop_oldest)
        del h
    return dict(append=statistics.median(times), append_all=times, pop_oldest=t_pop, rows=rows), first, max(peaks)


def same_rows(a_cols, b_cols):
    """the two paths' columns for one iteration are identical as sequences"""
    for a, b in zip(a_cols, b_cols):
        a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
        if a.shape != b.shape:
            return False
        if not torch.equal(a.to(b.dtype), b):
            return False
    return True


def measure(name, g, n_records, H, repeat, maxlen=10 ** 6):
    recs = synthetic_records(g, n_records)
    small = [t[:64].contiguous() for t in recs]
    default_path(g, small, 1, maxlen)                     # warm-up: code objects, allocator
    device_path(g, small, 2, maxlen, 1)
    # both paths give the same rows in the same order (before the default path's shuffle)
    from azg_amd.coach import Coach
    ex = Coach._collect(types.SimpleNamespace(game=g, dist=None, _sym_stream=0), [tuple(recs)])
    dev, first, peak_b = device_path(g, recs, H, maxlen, repeat)
    assert same_rows(ex[:5], first), 'the two paths disagree'
    del ex, first
    torch.cuda.empty_cache()
    dev1, _, _ = device_path(g, recs, 1, maxlen, repeat)
    a1, _, peak_a = default_path(g, recs, 1, maxlen)
    aH, _, _ = default_path(g, recs, H, maxlen)
    # like with like: the default path's peak holds its output (the compacted copy); the device path writes its output into the history's
    # own buffers, which were there before the call -- their share is added
    row_bytes = g.S + 4 * g.A + g.A + 8 * g.P
    return dict(game=name, records=n_records, rows=dev['rows'], history=H, default_h1=a1, default_hH=aH, device_h1=dev1, device_hH=dev,
                peak_bytes_default=int(peak_a), peak_bytes_device=int(peak_b) + dev['rows'] * row_bytes, row_bytes=row_bytes)


def markdown(results):
    out = ['| game | records | rows | path | history | collect / expand | encode | decode + upload | total | peak MiB of the expansion |', '|---|---|---|---|---|---|---|---|---|---|']
    for r in results:
        for key, H in (('default_h1', 1), ('default_hH', r['history'])):
            d = r[key]
            out.append('| %s | %d | %d | default | %d | %.3f s | %.2f s | %.2f s | %.2f s | %.0f |' % (
                r['game'], r['records'], r['rows'], H, d['collect'], d['encode'], d['decode_upload'], d['total'], r['peak_bytes_default'] / 2 ** 20))
        for key, H in (('device_h1', 1), ('device_hH', r['history'])):
            d = r[key]
            out.append('| %s | %d | %d | device history | %d | %.4f s | - | - | %.4f s (+ pop_oldest %.4f s) | %.0f |' % (
                r['game'], r['records'], r['rows'], H, d['append'], d['append'], d['pop_oldest'], r['peak_bytes_device'] / 2 ** 20))
    return '\n'.join(out)


def graph_us(fn, calls=20, replays=20):
    """device time of one fn() in microseconds: `calls` of them captured in one graph, the graph replayed `replays` times between two events"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            fn()
    graph.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(replays):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (calls * replays)


def measure_compact(name, g, n_records, repeat, batch):
    from azg_amd import train
    from azg_amd.history import CompactHistory, DeviceHistory
    recs = synthetic_records(g, n_records)
    s0 = 1 << 42
    small = [t[:64].contiguous() for t in recs]
    DeviceHistory(g.S, g.A, g.P, device=g.device).append_records(g, small, stream0=s0)                # warm-up: code objects, allocator
    probe = CompactHistory(g.S, g.A, g.P, device=g.device)
    rows, _ = probe.append_records(g, recs, stream0=s0)
    del probe
    t_dev, t_cmp = [], []
    for _ in range(repeat):                                                                           # alternating, buffers allocated before
        d = DeviceHistory(g.S, g.A, g.P, device=g.device, capacity=rows)
        t_dev.append(timed(lambda: d.append_records(g, recs, stream0=s0))[0])
        c = CompactHistory(g.S, g.A, g.P, device=g.device, capacity=n_records)
        t_cmp.append(timed(lambda: c.append_records(g, recs, stream0=s0))[0])
    assert d.n == c.n == rows
    gen = torch.Generator(device='cpu').manual_seed(3)
    check = torch.randint(0, rows, (4096,), generator=gen).to(torch.int32).to(g.device)
    cols = d.columns()
    assert same_rows(c.gather(check), [x[check.long()] for x in cols]), 'the compact history gives other rows'
    row_bytes = g.S + 4 * g.A + g.A + 8 * g.P
    assert c.device_bytes() == n_records * (row_bytes + 24) and sum(x.numel() * x.element_size() for x in cols) == rows * row_bytes
    ids = torch.randint(0, rows, (batch,), generator=gen).to(torch.int32).to(g.device)
    outs = train.gather_batch(cols, ids)
    k_exp, k_cmp = [], []
    for _ in range(2):                                                                                # alternating
        k_exp.append(graph_us(lambda: train.gather_batch(cols, ids, out=outs)))
        k_cmp.append(graph_us(lambda: c.gather(ids, out=outs)))
    return dict(game=name, records=n_records, rows=rows, forms_per_record=rows / n_records, batch=batch, append_device_s=t_dev, append_compact_s=t_cmp,
                gather_us=k_exp, gather_forms_us=k_cmp, bytes_device=rows * row_bytes, bytes_compact=c.device_bytes(), row_bytes=row_bytes)


def markdown_compact(results):
    out = ['| game | records | rows | forms / record | device history MiB | compact history MiB | `DeviceHistory.append_records` (s), per run | '
           '`CompactHistory.append_records` (s), per run | `azg_train_gather`, B = %d (µs), per run | `azg_train_gather_forms`, B = %d (µs), per run | d = difference of the medians (µs) |'
           % (results[0]['batch'], results[0]['batch']), '|---|---|---|---|---|---|---|---|---|---|---|']
    fmt = lambda xs, f: ' / '.join(f % x for x in xs)  # noqa: E731
    for r in results:
        out.append('| %s | %d | %d | %.1f | %.1f | %.1f | %s | %s | %s | %s | %.1f |' % (
            r['game'], r['records'], r['rows'], r['forms_per_record'], r['bytes_device'] / 2 ** 20, r['bytes_compact'] / 2 ** 20,
            fmt(r['append_device_s'], '%.4f'), fmt(r['append_compact_s'], '%.4f'), fmt(r['gather_us'], '%.1f'), fmt(r['gather_forms_us'], '%.1f'),
            statistics.median(r['gather_forms_us']) - statistics.median(r['gather_us'])))
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--compact', action='store_true', help='the compact history against the device history (see above)')
    ap.add_argument('--records-splendor', type=int, default=None, help='default 8192; 32768 with --compact')
    ap.add_argument('--records-azul', type=int, default=None, help='default 1024; 4096 with --compact')
    ap.add_argument('--records-tlp', type=int, default=8192, help='The Little Prince, 3 players (--compact only)')
    ap.add_argument('--batch', type=int, default=512, help='rows of the timed batch (--compact only)')
    ap.add_argument('--history', type=int, default=5, help='numItersHistory of the long case')
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--out', default=None, help='write the markdown table and the JSON lines here as well')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_history.py measures on the GPU: no device found')
    from azg_amd import games
    results = []
    if a.compact:
        for name, make, n in (('Splendor-2p', lambda: games.SplendorGame(2), 32768 if a.records_splendor is None else a.records_splendor),
                              ('Azul', games.AzulGame, 4096 if a.records_azul is None else a.records_azul),
                              ('The Little Prince 3p', lambda: games.TLPGame(num_players=3), a.records_tlp)):
            if n > 0:
                results.append(measure_compact(name, make(), n, a.repeat, a.batch))
                print(json.dumps(results[-1]), flush=True)
                torch.cuda.empty_cache()
        text = markdown_compact(results)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write(text + '\n\n' + '\n'.join(json.dumps(r) for r in results) + '\n')
        return
    a.records_splendor = 8192 if a.records_splendor is None else a.records_splendor
    a.records_azul = 1024 if a.records_azul is None else a.records_azul
    for name, g, n in (('Splendor-2p', games.SplendorGame(2), a.records_splendor), ('Azul', games.AzulGame(), a.records_azul)):
        if n > 0:
            results.append(measure(name, g, n, a.history, a.repeat))
            print(json.dumps(results[-1]), flush=True)
    text = markdown(results)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n\n' + '\n'.join(json.dumps(r) for r in results) + '\n')


if __name__ == '__main__':
    main()
