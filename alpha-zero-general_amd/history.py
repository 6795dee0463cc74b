"""Coach's example history as five preallocated column buffers on one device (Coach(device_history=True)):

    boards int8[cap, S]   pi f32[cap, A]   z f32[cap, P]   valids u8[cap, A]   q f32[cap, P]

The live rows are always the prefix [0, n): iteration i owns rows [sum(sizes[:i]), sum(sizes[:i + 1])).  An iteration's drained
records go from the forest's ring into the rows behind n with two launches of azg_examples_expand (csrc/examples.hip.h): a count
pass, a prefix sum with the one host read of the total, and a write pass -- no [n, K, .] intermediate, no mask, nothing on the host.
train.train(history.columns(), device_batches=True) reads the prefix in place.  Everything except append_records is plain torch and
works on CPU tensors as well; the reference's file formats go through formats.examples_to_iteration.

CompactHistory (Coach(device_history='compact')) keeps the records instead and lets the gather of a training batch compute the forms
it names (azg_train_gather_forms): the same rows at 1 / forms-per-record of the memory."""
import pickle
import zlib

import numpy as np
import torch

from . import formats

_DTYPES = (torch.int8, torch.float32, torch.float32, torch.uint8, torch.float32)
_NAMES = ('boards', 'pi', 'z', 'valids', 'q')
_NP_DTYPES = (np.int8, np.float32, np.float32, np.uint8, np.float32)
_INDEX_NAMES =('first_row', 'row_end', 'stream')
ROWS_CHUNK = 65536                                      # CompactHistory.rows materialises at most this many rows per launch


def _canonical_order(meta):
    """the order of Coach._collect: ply, then game index, then stream (three stable sorts) -> int64 permutation"""
    m = meta.to(torch.int64)
    order = torch.argsort(m[:, 2], stable=True)
    order = order[torch.argsort(m[order, 1], stable=True)]
    return order[torch.argsort(m[order, 0], stable=True)]


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


class CompactHistory:
    """The same history as DeviceHistory with the RECORDS stored instead of their symmetric forms (Coach(device_history='compact')):

        boards int8[cap, S]   pi f32[cap, A]   z f32[cap, P]   valids u8[cap, A]   q f32[cap, P]      one row per record
        first_row i64[cap]    row_end i64[cap]   stream i64[cap]                                         24 bytes per record

    The rows DeviceHistory would hold exist as VIRTUAL rows [0, n): form k of record g is virtual row first_row[g] + k, the record's
    live rows end at row_end[g] (non-decreasing in g), and its forms draw from stream (rng_seed, stream[g]).  Virtual row r is defined to
    be row r of the expanded history; azg_train_gather_forms (csrc/examples.hip.h) computes the rows a batch names from the records, so
    the trainer reads the same bytes and the memory falls by the forms-per-record factor.  Iteration i owns virtual rows
    [sum(sizes[:i]), sum(sizes[:i + 1])) and records [sum(rec_sizes[:i]), sum(rec_sizes[:i + 1])).  The bookkeeping is plain torch and
    works on CPU tensors (append_counted); append_records, gather and everything that materialises rows need the GPU."""

    def __init__(self, S, A, P, device='cpu', capacity=0):
        """capacity: records to allocate up front; the buffers grow to at least double when an append needs more"""
        self.S, self.A, self.P = int(S), int(A), int(P)
        self.device = torch.device(device)
        self.sizes = []                                   # virtual rows of every iteration, oldest first
        self.rec_sizes = []                               # records of every iteration
        self.n = 0                                        # live virtual rows = sum(sizes)
        self.n_records = 0                                # stored records = sum(rec_sizes)
        self.game_id = self.variant = self.rng_seed = None     # fixed by the first append
        self.capacity = 0
        self._bufs = None
        self._alloc(max(0, int(capacity)))

    @property
    def widths(self):
        return (self.S, self.A, self.P, self.A, self.P)

    @property
    def row_bytes(self):
        """bytes of one record = of one expanded row"""
        return self.S + 4 * self.A + 4 * self.P + self.A + 4 * self.P

    def _alloc(self, cap):
        new = tuple(torch.empty((cap, w), dtype=dt, device=self.device) for w, dt in zip(self.widths, _DTYPES)) + \
            tuple(torch.empty((cap,), dtype=torch.int64, device=self.device) for _ in _INDEX_NAMES)
        if self._bufs is not None and self.n_records:
            for dst, src in zip(new, self._bufs):
                dst[:self.n_records].copy_(src[:self.n_records])
        self._bufs, self.capacity = new, cap

    def reserve(self, records):
        """room for `records` stored records"""
        if records > self.capacity:
            self._alloc(max(int(records), 2 * self.capacity))

    def __len__(self):
        return len(self.sizes)

    def record_columns(self):
        """views of the stored records: the five columns"""
        return tuple(b[:self.n_records] for b in self._bufs[:5])

    def index_columns(self):
        """views of (first_row, row_end, stream) of the stored records"""
        return tuple(b[:self.n_records] for b in self._bufs[5:])

    def device_bytes(self):
        """live device bytes: the stored records and their 24 bytes of index"""
        return self.n_records * (self.row_bytes + 24)

    def _bind(self, game):
        gid, var, seed = int(game.GAME_ID), int(game.variant), int(game.rng_seed)
        if self.rng_seed is None:
            self.game_id, self.variant, self.rng_seed = gid, var, seed
        elif (gid, var) != (self.game_id, self.variant):
            raise ValueError('CompactHistory: records of game (%d, %d) appended to a history of game (%d, %d)' % (gid, var, self.game_id, self.variant))
        elif seed != self.rng_seed:
            raise ValueError('CompactHistory: the history draws its forms with rng_seed %d (fixed by the first append), this game has rng_seed %d: '
                             'the rows already appended would change' % (self.rng_seed, seed))

    # ---- appending ----
    def append_counted(self, game, records, counts, maxlen=None, stream0=0):
        """One iteration from records that are in their final order and the number of forms of each (int tensor [n]): no row is written,
        the records and their index entries are appended.  Record t draws from stream stream0 + t.  maxlen keeps the LAST maxlen virtual
        rows: first_row keeps its true value (below the iteration's base for a record cut in the middle), row_end is clamped from below
        to the base -- a record that is wholly cut owns no row.  One host read (the total).  -> (rows kept, rows before the cut)"""
        self._bind(game)
        cols = [x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x)) for x in records[:5]]
        n = int(cols[0].shape[0])
        if n == 0:
            self.sizes.append(0)
            self.rec_sizes.append(0)
            return 0, 0
        cnt = counts.to(self.device).to(torch.int64).reshape(n)
        ends = torch.cumsum(cnt, dim=0)
        total = int(ends[-1].item())                                       # the one host read
        kept = total if maxlen is None else min(total, max(0, int(maxlen)))
        base = self.n
        first_row = ends - cnt + (base - (total - kept))
        row_end = torch.clamp(first_row + cnt, min=base)
        stream = torch.arange(n, dtype=torch.int64, device=self.device) + _as_i64(stream0)
        self.reserve(self.n_records + n)
        a, b = self.n_records, self.n_records + n
        for j, (buf, x, w) in enumerate(zip(self._bufs, cols, self.widths)):
            x = x.reshape(n, w).to(self.device)
            x = (x != 0) if j == 3 else x                                  # valids: bool or 0 / non-zero bytes -> 0 / 1
            buf[a:b].copy_(x.to(buf.dtype))
        for buf, x in zip(self._bufs[5:], (first_row, row_end, stream)):
            buf[a:b].copy_(x)
        self.sizes.append(kept)
        self.rec_sizes.append(n)
        self.n += kept
        self.n_records += n
        return kept, total

    def append_records(self, game, records, maxlen=None, stream0=0):
        """DeviceHistory.append_records without the write pass: the canonical order, the count pass of azg_examples_expand on the streams
        (game.rng_seed, stream0 + t), one prefix sum, the one host read of the total -- then append_counted.  -> (rows kept, rows before
        the cut), the same numbers DeviceHistory returns"""
        from .games import _ptr, _stream
        from ._lib import check, lib
        self._bind(game)
        boards, pi, z, valids, q, meta = records[:6]
        n = int(boards.shape[0])
        if n == 0:
            return self.append_counted(game, (boards, pi, z, valids, q), None, maxlen, stream0)
        if self.device.type != 'cuda' or boards.device != self.device:
            raise ValueError('append_records: the records (%s) and the history (%s) must be on one CUDA device' % (boards.device, self.device))
        order = _canonical_order(meta)
        boards = boards.reshape(n, self.S)[order].contiguous()
        pi, z, q = pi[order].contiguous(), z[order].contiguous(), q[order].contiguous()
        valids = (valids if valids.dtype == torch.uint8 else valids.to(torch.uint8))[order].contiguous()
        assert boards.dtype == torch.int8 and pi.dtype == z.dtype == q.dtype == torch.float32
        assert pi.shape == (n, self.A) and valids.shape == (n, self.A) and z.shape == (n, self.P) and q.shape == (n, self.P)
        cnt = torch.zeros((n,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().azg_examples_expand(game.GAME_ID, game.variant, _ptr(boards), _ptr(pi), _ptr(z), _ptr(valids), _ptr(q), n, None, None,
                                            0, 0, None, None, None, None, None, _ptr(cnt), self.rng_seed, int(stream0), _stream()))
        return self.append_counted(game, (boards, pi, z, valids, q), cnt, maxlen, stream0)

    # ---- dropping ----
    def pop_oldest(self):
        """drop the first iteration: its records leave, the records behind them move to the front and every index entry is rebased by
        the dropped rows -> the dropped rows"""
        k, r = self.sizes.pop(0), self.rec_sizes.pop(0)
        rest = self.n_records - r
        if r and rest:
            for b in self._bufs:
                for a in range(0, rest, r):                               # front-to-back pieces of the dropped size: no overlap
                    e = min(a + r, rest)
                    b[a:e].copy_(b[a + r:e + r])
        self.n_records = rest
        self.n -= k
        if k and rest:
            self._bufs[5][:rest] -= k
            self._bufs[6][:rest] -= k
        return k

    def truncate_iteration(self, i, rows):
        """keep the first `rows` virtual rows of iteration i: row_end of its records is clamped from above, the records behind it are
        rebased.  (The records that lose every row stay stored; they own no row.)"""
        i = range(len(self.sizes))[i]
        drop = self.sizes[i] - max(0, int(rows))
        if drop <= 0:
            return
        end = sum(self.sizes[:i + 1]) - drop                               # the iteration's new end
        ra, rb = sum(self.rec_sizes[:i]), sum(self.rec_sizes[:i + 1])
        first_row, row_end = self._bufs[5], self._bufs[6]
        row_end[ra:rb].clamp_(max=end)
        first_row[rb:self.n_records] -= drop
        row_end[rb:self.n_records] -= drop
        self.sizes[i] -= drop
        self.n -= drop

    # ---- reading rows ----
    def gather(self, ids, out=None):
        """virtual rows `ids` (int32[B], on the device) -> (boards int8[B, S], pi, z, valids u8[B, A] holding 0 / 1, q): one launch of
        azg_train_gather_forms, nothing synchronised, nothing allocated when `out` is given.  An id outside [0, n) gives an undefined row."""
        from .train import gather_forms
        if self.n_records == 0:
            raise ValueError('CompactHistory.gather: the history holds no record')
        return gather_forms(self.game_id, self.variant, self.record_columns(), *self.index_columns(), ids, self.rng_seed, out=out)

    def rows(self, lo, hi):
        """virtual rows [lo, hi) materialised as the five columns: gather on an arange, at most ROWS_CHUNK rows per launch"""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi <= self.n:
            raise ValueError('CompactHistory.rows: [%d, %d) is not inside the %d live rows' % (lo, hi, self.n))
        out = tuple(torch.empty((hi - lo, w), dtype=dt, device=self.device) for w, dt in zip(self.widths, _DTYPES))
        for a in range(lo, hi, ROWS_CHUNK):
            b = min(a + ROWS_CHUNK, hi)
            self.gather(torch.arange(a, b, dtype=torch.int32, device=self.device), out=tuple(o[a - lo:b - lo] for o in out))
        return out

    def columns(self):
        """every live row, materialised (DeviceHistory.columns() as new tensors)"""
        return self.rows(0, self.n)

    def iteration_columns(self, i):
        i = range(len(self.sizes))[i]
        a = sum(self.sizes[:i])
        return self.rows(a, a + self.sizes[i])

    def iteration_valid_moves(self, i):
        """the number of valid moves summed over the rows of iteration i (one chunk of rows at a time)"""
        i = range(len(self.sizes))[i]
        a = sum(self.sizes[:i])
        total = 0
        for lo in range(a, a + self.sizes[i], ROWS_CHUNK):
            total += int(self.rows(lo, min(lo + ROWS_CHUNK, a + self.sizes[i]))[3].sum(dtype=torch.int64).item())
        return total

    def to_reference(self, i, board_shape, compress=True, maxlen=None):
        """the deque of iteration i as Coach.executeEpisodes builds it (formats.examples_to_iteration), from its materialised rows"""
        return formats.examples_to_iteration(self.iteration_columns(i), tuple(board_shape), compress=compress, maxlen=maxlen)

    def save_columns(self, path):
        """DeviceHistory.save_columns' file from the materialised rows, one iteration on the device at a time"""
        parts = [[c.cpu().numpy() for c in self.iteration_columns(i)] for i in range(len(self.sizes))]
        arrs = {name: (np.concatenate([p[k] for p in parts]) if parts else np.zeros((0, w), dtype=_NP_DTYPES[k]))
                for k, (name, w) in enumerate(zip(_NAMES, self.widths))}
        with open(path, 'wb') as f:
            np.savez(f, sizes=np.asarray(self.sizes, dtype=np.int64), **arrs)

    # ---- the records as one file ----
    def save_records(self, path):
        """one uncompressed np.savez: the record and index columns, both lists of sizes, the game and its rng_seed"""
        arrs = {name: c.cpu().numpy() for name, c in zip(_NAMES + _INDEX_NAMES, self.record_columns() + self.index_columns())}
        with open(path, 'wb') as f:
            np.savez(f, sizes=np.asarray(self.sizes, dtype=np.int64), rec_sizes=np.asarray(self.rec_sizes, dtype=np.int64),
                     game=np.asarray([-1 if self.game_id is None else self.game_id, -1 if self.variant is None else self.variant], dtype=np.int64),
                     rng_seed=np.asarray([0 if self.rng_seed is None else self.rng_seed], dtype=np.uint64), **arrs)

    @classmethod
    def load_records(cls, path, device='cpu', capacity=0):
        with np.load(path) as d:
            if 'first_row' not in d.files:
                raise ValueError('%s holds expanded columns, not records: load it with DeviceHistory.load_columns' % path)
            cols = [d[name] for name in _NAMES + _INDEX_NAMES]
            sizes, rec_sizes = [int(s) for s in d['sizes']], [int(s) for s in d['rec_sizes']]
            game, seed = [int(x) for x in d['game']], int(d['rng_seed'][0])
        if sum(rec_sizes) != len(cols[0]) or len(sizes) != len(rec_sizes):
            raise ValueError('%s: the record counts %r do not add up to its %d records' % (path, rec_sizes, len(cols[0])))
        h = cls(cols[0].shape[1], cols[1].shape[1], cols[2].shape[1], device=device, capacity=max(int(capacity), len(cols[0])))
        for buf, x in zip(h._bufs, cols):
            buf[:len(x)].copy_(torch.from_numpy(np.ascontiguousarray(x)))
        h.sizes, h.rec_sizes, h.n, h.n_records = sizes, rec_sizes, sum(sizes), sum(rec_sizes)
        if game[0] >= 0:
            h.game_id, h.variant, h.rng_seed = game[0], game[1], seed
        return h


def _as_i64(x):
    """a stream number (up to 2^64 - 1) as the int64 with the same bits"""
    x = int(x) & (2 ** 64 - 1)
    return x - 2 ** 64 if x >= 2 ** 63 else x
