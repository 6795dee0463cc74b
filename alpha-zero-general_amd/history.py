"""Coach's example history as five preallocated column buffers on one device (Coach(device_history=True)):

    boards int8[cap, S]   pi f32[cap, A]   z f32[cap, P]   valids u8[cap, A]   q f32[cap, P]

The live rows are always the prefix [0, n): iteration i owns rows [sum(sizes[:i]), sum(sizes[:i + 1])).  An iteration's drained
records go from the forest's ring into the rows behind n with two launches of azg_examples_expand (csrc/examples.hip.h): a count
pass, a prefix sum with the one host read of the total, and a write pass -- no [n, K, .] intermediate, no mask, nothing on the host.
train.train(history.columns(), device_batches=True) reads the prefix in place.  Everything except append_records is plain torch and
works on CPU tensors as well; the reference's file formats go through formats.examples_to_iteration."""
import pickle
import zlib

import numpy as np
import torch

from . import formats

_DTYPES = (torch.int8, torch.float32, torch.float32, torch.uint8, torch.float32)
_NAMES = ('boards', 'pi', 'z', 'valids', 'q')


class DeviceHistory:
    def __init__(self, S, A, P, device='cpu', capacity=0):
        """capacity: rows to allocate up front; the buffers grow to at least double when an append needs more (one device copy per
        column) -- rows are never dropped"""
        self.S, self.A, self.P = int(S), int(A), int(P)
        self.device = torch.device(device)
        self.sizes = []                                   # rows of every iteration, oldest first
        self.n = 0                                        # live rows = sum(sizes)
        self.capacity = 0
        self._bufs = None
        self._alloc(max(0, int(capacity)))

    @property
    def widths(self):
        return (self.S, self.A, self.P, self.A, self.P)

    def _alloc(self, cap):
        new = tuple(torch.empty((cap, w), dtype=dt, device=self.device) for w, dt in zip(self.widths, _DTYPES))
        if self._bufs is not None and self.n:
            for dst, src in zip(new, self._bufs):
                dst[:self.n].copy_(src[:self.n])
        self._bufs, self.capacity = new, cap

    def reserve(self, rows):
        """room for `rows` live rows"""
        if rows > self.capacity:
            self._alloc(max(int(rows), 2 * self.capacity))

    def __len__(self):
        return len(self.sizes)

    def columns(self):
        """views of the n live rows of the five columns (contiguous: a prefix of contiguous buffers)"""
        return tuple(b[:self.n] for b in self._bufs)

    def iteration_columns(self, i):
        i = range(len(self.sizes))[i]
        a = sum(self.sizes[:i])
        return tuple(b[a:a + self.sizes[i]] for b in self._bufs)

    # ---- appending ----
    def append_columns(self, cols):
        """one iteration of rows that are already expanded (a loaded file, another history): five arrays / tensors -> rows appended"""
        cols = [x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x)) for x in cols[:5]]
        k = int(cols[0].shape[0])
        self.reserve(self.n + k)
        for j, (buf, x, w) in enumerate(zip(self._bufs, cols, self.widths)):
            x = x.reshape(k, w)
            x = (x != 0) if j == 3 else x                                    # valids: bool or 0 / non-zero bytes -> 0 / 1
            buf[self.n:self.n + k].copy_(x.to(self.device).to(buf.dtype))
        self.sizes.append(k)
        self.n += k
        return k

    def append_records(self, game, records, maxlen=None, stream0=0):
        """One iteration from its drained (and gathered) records (boards, pi, z, valids, q, meta) on the history's device: canonical
        order (stream, game index, ply -- the three stable sorts of Coach._collect), every symmetric form of every record, record t of
        that order drawing from stream (game.rng_seed, stream0 + t).  maxlen is deque(maxlen=maxlenOfQueue) fed in order: when the
        iteration has more rows, its LAST maxlen are kept.  -> (rows kept, rows before the cut)"""
        from .games import _ptr, _stream
        from ._lib import check, lib
        boards, pi, z, valids, q, meta = records[:6]
        n = int(boards.shape[0])
        if n == 0:
            self.sizes.append(0)
            return 0, 0
        if self.device.type != 'cuda' or boards.device != self.device:
            raise ValueError('append_records: the records (%s) and the history (%s) must be on one CUDA device' % (boards.device, self.device))
        boards = boards.reshape(n, self.S).contiguous()
        pi, z, q = pi.contiguous(), z.contiguous(), q.contiguous()
        valids = (valids if valids.dtype == torch.uint8 else valids.to(torch.uint8)).contiguous()
        assert boards.dtype == torch.int8 and pi.dtype == z.dtype == q.dtype == torch.float32
        assert pi.shape == (n, self.A) and valids.shape == (n, self.A) and z.shape == (n, self.P) and q.shape == (n, self.P)
        m = meta.to(torch.int64)
        order = torch.argsort(m[:, 2], stable=True)                       # ply, then game index, then stream (stable sorts)
        order = order[torch.argsort(m[order, 1], stable=True)]
        order = order[torch.argsort(m[order, 0], stable=True)]
        order = order.to(torch.int32).contiguous()
        cnt = torch.zeros((n,), dtype=torch.int32, device=self.device)
        seed = int(game.rng_seed)

        def expand(first_row, lo, hi):
            with torch.cuda.device(self.device):
                check(lib().azg_examples_expand(game.GAME_ID, game.variant, _ptr(boards), _ptr(pi), _ptr(z), _ptr(valids), _ptr(q), n,
                                                _ptr(order), _ptr(first_row), lo, hi, *[_ptr(b) for b in self._bufs], _ptr(cnt), seed,
                                                int(stream0), _stream()))

        expand(None, 0, 0)                                                 # the count pass
        ends = torch.cumsum(cnt, dim=0, dtype=torch.int64)
        total = int(ends[-1].item())                                       # the one host read
        kept = total if maxlen is None else min(total, int(maxlen))
        self.reserve(self.n + kept)                                        # (before the pointers of the write pass are taken)
        first_row = (ends - cnt + (self.n - (total - kept))).contiguous()
        expand(first_row, self.n, self.n + kept)
        self.sizes.append(kept)
        self.n += kept
        return kept, total

    # ---- dropping ----
    def pop_oldest(self):
        """drop the first iteration; the rows behind it move to the front, so the live rows stay the prefix.  The move is one copy per
        column where source and destination do not overlap, and front-to-back pieces of the dropped size where they do"""
        k = self.sizes.pop(0)
        rest = self.n - k
        if k and rest:
            for b in self._bufs:
                for a in range(0, rest, k):
                    e = min(a + k, rest)
                    b[a:e].copy_(b[a + k:e + k])
        self.n = rest
        return k

    def truncate_iteration(self, i, rows):
        """keep the first `rows` rows of iteration i (loadTrainExamples' `while len(it) > maxlen: it.pop()`)"""
        i = range(len(self.sizes))[i]
        drop = self.sizes[i] - int(rows)
        if drop <= 0:
            return
        a = sum(self.sizes[:i + 1])                                        # first row behind iteration i
        for b in self._bufs:
            if self.n > a:
                b[a - drop:self.n - drop].copy_(b[a:self.n].clone())
        self.sizes[i] -= drop
        self.n -= drop

    # ---- the reference's layout ----
    def to_reference(self, i, board_shape, compress=True, maxlen=None):
        """the deque of iteration i as Coach.executeEpisodes builds it (formats.examples_to_iteration)"""
        return formats.examples_to_iteration(self.iteration_columns(i), tuple(board_shape), compress=compress, maxlen=maxlen)

    @classmethod
    def from_reference(cls, history, device='cpu', capacity=0, widths=None):
        """a list of iterations (deques or lists of 5-tuples, or of their zlib-compressed pickles) -> DeviceHistory.  widths = (S, A, P);
        None takes them from the first example"""
        decoded = [[e if isinstance(e, tuple) else pickle.loads(zlib.decompress(e)) for e in it] for it in history]
        if widths is None:
            first = next((it[0] for it in decoded if it), None)
            if first is None:
                raise ValueError('from_reference: a history without examples needs widths=(S, A, P)')
            widths = (np.asarray(first[0]).size, np.asarray(first[1]).size, np.asarray(first[2]).size)
        h = cls(*widths, device=device, capacity=max(int(capacity), sum(len(it) for it in decoded)))
        for ex in decoded:
            if not ex:
                h.sizes.append(0)
                continue
            h.append_columns([np.stack([np.asarray(e[k]).reshape(-1) for e in ex]) for k in range(5)])
        return h

    # ---- the columns as one file ----
    def save_columns(self, path):
        """one uncompressed np.savez: the five columns' live rows and the iteration sizes"""
        arrs = {name: c.cpu().numpy() for name, c in zip(_NAMES, self.columns())}
        with open(path, 'wb') as f:
            np.savez(f, sizes=np.asarray(self.sizes, dtype=np.int64), **arrs)

    @classmethod
    def load_columns(cls, path, device='cpu', capacity=0):
        with np.load(path) as d:
            cols = [d[name] for name in _NAMES]
            sizes = [int(s) for s in d['sizes']]
        if sum(sizes) != len(cols[0]):
            raise ValueError('%s: the sizes %r do not add up to its %d rows' % (path, sizes, len(cols[0])))
        h = cls(cols[0].shape[1], cols[1].shape[1], cols[2].shape[1], device=device, capacity=max(int(capacity), len(cols[0])))
        a = 0
        for s in sizes:
            if s:
                h.append_columns([c[a:a + s] for c in cols])
            else:
                h.sizes.append(0)
            a += s
        return h
