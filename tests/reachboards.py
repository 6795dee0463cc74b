"""Boards for the net tests from every reachable position (a helper module of tests/test_net_reachable_boards.py and
tests/test_gpu_net_reachable_boards.py, not a conftest): the net kernels are the only hot-path code whose behaviour depends on the bytes
of the board, and tests/golden/netfwd_<tag>.npz holds early and mid-game positions only.

CPU only (numpy, torch, azg_oracle); nothing new is stored: the inputs are the committed env-coverage fixtures.

    batch(tag) -> (boards int8 [n, ...board shape], masks uint8 [n, A], meta)

for every tag of netweights.configs() and the two further shipped Abalone nets (EXTRA):
  boards   the `canonical` field of tests/golden/envcover_<variant>.npz, every row: the canonical form of the position after each covering
           move, last transitions of finished games included.  An Abalone net takes both files of its set-up (the steered games and the
           games won by six); Botanik V10 and V11 share one file;
  masks    the oracle's getValidMoves(canonical, 0), what the search asks of a leaf;
  edited   two rows as in netweights.boards (copies of the two fixture rows with the most valid actions): one with an all-zero mask, one
           with a single valid action.  Akropolis: eight more, copies of evenly spaced rows of finished games with description codes
           overwritten by CODE_EDITS (the reference clamps a code to 0..11): four with cells of every player's description plane, four
           with the construction-site codes as well;
  meta     per row `file`, `row` (the fixture's `row`: the index in envcover.rows), `index` (the row in the file), `group`, `ended`
           (the game is over in that position) and `edit` ('' for a fixture row), so that a failure can name them."""
import functools
import os

import numpy as np
import torch

import envcover as E
import netweights as nw

GOLDEN = nw.GOLDEN
# shipped nets that are no netweights config of their own (the Abalone V21 row with the checkpoint of another layout): shipped weights only
EXTRA = {'abalone_v21_classic': 'abalone_v21', 'abalone_v21_german': 'abalone_v21'}
CODE_EDITS = (-128, -1, 12, 127)
EDIT_ROWS = 8                  # Akropolis: rows with edited description codes
EDIT_STRIDE = 7                # ... every 7th cell of each player's description plane (25 of 169: borders, corners, interior)


def tags():
    return [c.tag for c in nw.configs()] + list(EXTRA)


def config(tag):
    """the netweights Config of a tag; for a tag of EXTRA the row of its base config under its own tag (fixture, shipped weights)"""
    if tag in EXTRA:
        return nw.config(EXTRA[tag])._replace(tag=tag)
    return nw.config(tag)


def variants(tag):
    """the env-coverage variants (envcover_<variant>.npz) whose positions a net evaluates"""
    stem = tag.rsplit('_v', 1)[0]
    if stem == 'abalone':
        layout = tag.split('_v21')[1]                         # '', '_classic', '_german'
        return ['abalone' + layout, 'abalone' + layout + '_six']
    return [stem]


def oracle_variant(variant):
    return variant[:-len('_six')] if variant.endswith('_six') else variant


@functools.lru_cache(maxsize=None)
def _fixture_rows(variant):
    """(canonical int8 [n, S], masks uint8 [n, A], row, group, ended) of one fixture file"""
    d = np.load(os.path.join(GOLDEN, 'envcover_%s.npz' % variant))
    og = E.oracle_game(oracle_variant(variant))
    canon = np.ascontiguousarray(d['canonical'])
    masks = np.array([og.getValidMoves(c.reshape(og.shape), 0) for c in canon], dtype=np.uint8).reshape(len(canon), og.A)
    return canon, masks, d['row'].astype(np.int64), d['group'].astype(np.int64), d['ended'].any(axis=1)


def akropolis_code_cells(P):
    """(flat indices of the description cells of the players' planes that the edited rows overwrite, of the construction-site codes):
    board int8 [13][13][3P + 2], descriptions in channels 0..P-1, site codes in channel 3P + 1 at rows 0..P+1, columns 0..2"""
    C = 3 * P + 2
    planes = np.array([cell * C + p for p in range(P) for cell in range(p, 169, EDIT_STRIDE)], dtype=np.int64)
    sites = np.array([(c * 13 + k) * C + 3 * P + 1 for c in range(P + 2) for k in range(3)], dtype=np.int64)
    return planes, sites


@functools.lru_cache(maxsize=None)
def _batch(tag):
    cfg = config(tag)
    P, A = nw.shape(cfg)
    parts = [_fixture_rows(v) + (v,) for v in variants(tag)]
    canon = np.concatenate([p[0] for p in parts])
    masks = np.concatenate([p[1] for p in parts])
    meta = dict(file=np.concatenate([np.full(len(p[0]), 'envcover_%s.npz' % p[5]) for p in parts]),
                row=np.concatenate([p[2] for p in parts]), index=np.concatenate([np.arange(len(p[0])) for p in parts]),
                group=np.concatenate([p[3] for p in parts]), ended=np.concatenate([p[4] for p in parts]))
    n = len(canon)
    assert masks.shape == (n, A) and canon.shape[1] == int(np.prod(nw._fixture(tag)[0].shape[1:]))
    meta['edit'] = np.full(n, '', dtype='U24')
    src, new_b, new_m, edit = [], [], [], []
    # the two rows of netweights.boards, on copies of the two rows with the most valid actions (ties: the earlier row)
    most = np.argsort(-masks.sum(axis=1).astype(np.int64), kind='stable')[:2]
    src.append(int(most[0])); new_b.append(canon[most[0]]); new_m.append(np.zeros(A, dtype=np.uint8)); edit.append('no valid action')
    one = np.zeros(A, dtype=np.uint8)
    one[int(masks[most[1]].argmax())] = 1
    src.append(int(most[1])); new_b.append(canon[most[1]]); new_m.append(one); edit.append('one valid action')
    if tag.startswith('akropolis'):
        planes, sites = akropolis_code_cells(P)
        late = np.flatnonzero(meta['ended'])                 # finished games: full cities, so that a code clamped to 0 changes cells
        for j, r in enumerate(late[np.linspace(0, len(late) - 1, EDIT_ROWS).astype(np.int64)]):
            b = canon[r].copy()
            value = CODE_EDITS[j % 4]
            b[planes] = value
            if j >= 4:
                b[sites] = value
            src.append(int(r)); new_b.append(b); new_m.append(masks[r]); edit.append('codes %d%s' % (value, ' sites too' if j >= 4 else ''))
    src = np.array(src)
    canon = np.concatenate([canon, np.array(new_b, dtype=np.int8)])
    masks = np.concatenate([masks, np.array(new_m, dtype=np.uint8)])
    meta = {k: np.concatenate([v, v[src]]) for k, v in meta.items()}
    meta['edit'][n:] = edit
    meta['source'] = np.concatenate([np.arange(n), src])      # the batch row an edited row was copied from
    shape = tuple(nw._fixture(tag)[0].shape[1:])
    return canon.reshape((len(canon),) + shape), masks, meta


def batch(tag):
    """(boards int8 tensor [n, ...], masks uint8 tensor [n, A], meta: dict of arrays of length n); fresh tensors of cached arrays"""
    b, m, meta = _batch(tag)
    return torch.from_numpy(b.copy()), torch.from_numpy(m.copy()), meta


def name(meta, i):
    """what a failure says of batch row i"""
    i = int(i)
    edit = ', edited: %s' % meta['edit'][i] if meta['edit'][i] else ''
    return '%s index %d (row %d of rows(), group %d)%s' % (meta['file'][i], int(meta['index'][i]), int(meta['row'][i]), int(meta['group'][i]), edit)


def pairs(boards):
    """bool [cells, 256]: which (cell, value + 128) pairs occur in int8 boards [n, ...]"""
    flat = np.asarray(boards).reshape(len(boards), -1)
    seen = np.zeros((flat.shape[1], 256), dtype=bool)
    cells = np.arange(flat.shape[1])
    for r in flat:
        seen[cells, r.astype(np.int64) + 128] = True
    return seen


def new_pairs(tag):
    """bool [cells, 256]: the (cell, value) pairs of the fixture rows of batch(tag) that no row of netfwd_<tag>.npz has"""
    b, _, meta = _batch(tag)
    return pairs(b[meta['edit'] == '']) & ~pairs(nw._fixture(tag)[0])


@functools.lru_cache(maxsize=None)
def shipped(tag):
    """the trainable module with the shipped weights of the tag (Minivilles 4p and Botanik: the stand-ins, as they come), strict=True"""
    from azg_amd import formats
    cfg = config(tag)
    P, A = nw.shape(cfg)
    sd, _ = formats.fixture_state_dict(GOLDEN, tag)
    m = cfg.row.module(P, A, 0.0)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval()


def weight_sets(tag):
    return ('shipped',) if tag in EXTRA else ('shipped', 'calibrated')


def module(tag, weights):
    """a module of one of weight_sets(tag); the calibrated one is built anew at each call, the shipped one is shared: do not change it"""
    return shipped(tag) if weights == 'shipped' else nw.calibrated(config(tag))
