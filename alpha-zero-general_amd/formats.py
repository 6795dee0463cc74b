"""The reference's on-disk formats, so that engine output feeds the reference's trainer / tools and vice versa (host-side
data plumbing only, no compute):

* `checkpoint.examples` (Coach.saveTrainExamples / loadTrainExamples, Coach.py:215-262): `pickle.dump` of a list (one
  entry per iteration) of `deque(maxlen=maxlenOfQueue)` of examples; an example is the 5-tuple
  `(board int8 ndarray of getBoardSize(), pi, z = np.roll(result, -player), valids, q)` (Coach.py:76-82), stored either
  as is (`no_compression`) or as `zlib.compress(pickle.dumps(example), level=1)` (Coach.py:84).
* Arena initial-state string (Arena.py:61-65,91-93): `base64(raw-deflate(board bytes + player u8 + turn u16 big-endian))`.
* `.pt` checkpoints (GenericNNetWrapper.save_checkpoint :192-205): `torch.save({'state_dict', 'full_model', **args})`;
  reading one needs the reference's model classes importable because `full_model` is a pickled module."""
import base64
import pickle
import zlib
from collections import deque

import numpy as np


def examples_to_iteration(examples, board_shape, compress=True, maxlen=None):
    """(boards int8[n,S], pi f32[n,A], z f32[n,P], valids u8[n,A], q f32[n,P], ...) as returned by
    SelfPlayEngine.drain_examples() -> the deque of one self-play iteration in the reference's layout."""
    boards, pi, z, valids, q = [np.asarray(x.cpu() if hasattr(x, 'cpu') else x) for x in examples[:5]]
    out = deque([], maxlen=maxlen)
    for i in range(len(boards)):
        ex = (boards[i].reshape(board_shape).astype(np.int8), pi[i].astype(np.float32), z[i].astype(np.float32),
              valids[i].astype(bool), q[i].astype(np.float32))
        out.append(zlib.compress(pickle.dumps(ex), level=1) if compress else ex)
    return out


def save_train_examples(path, history):
    """history: list of iterations (deques) as built by examples_to_iteration; the file Coach.loadTrainExamples reads"""
    with open(path, 'wb') as f:
        pickle.dump(list(history), f)


def load_train_examples(path):
    """-> list of iterations, each a list of decompressed 5-tuples (board, pi, z, valids, q)"""
    with open(path, 'rb') as f:
        history = pickle.load(f)
    return [[ex if isinstance(ex, tuple) else pickle.loads(zlib.decompress(ex)) for ex in it] for it in history]


def encode_initial_state(board, player, turn):
    """the `state = "..."` string Arena prints in verbose mode and accepts as initial_state (Arena.py:61-65,91-93)"""
    data = np.ascontiguousarray(board, dtype=np.int8).tobytes() + int(player).to_bytes(1, 'big') + int(turn).to_bytes(2, 'big')
    c = zlib.compressobj(level=9, wbits=-15)
    return str(base64.b64encode(c.compress(data) + c.flush()), 'UTF-8')


def decode_initial_state(state, board_shape):
    """-> (board int8 ndarray, player, turn)"""
    data = zlib.decompress(base64.b64decode(state), wbits=-15)
    board = np.frombuffer(data[:-3], dtype=np.int8).reshape(board_shape).copy()
    return board, int(data[-3]), int.from_bytes(data[-2:], 'big')


def load_reference_checkpoint(path):
    """-> (state_dict of numpy arrays, dict of the scalar / list args embedded by save_checkpoint).  Needs the reference's
    package on sys.path (the pickled `full_model`); azg_amd.nnet.* accept the returned state_dict directly."""
    import torch
    ck = torch.load(path, map_location='cpu', weights_only=False)
    sd = {k: v.numpy() for k, v in ck['state_dict'].items()}
    args = {k: v for k, v in ck.items() if k not in ('state_dict', 'full_model')}
    return sd, args


# ---- stand-in weights for a shipped checkpoint too large to keep as a test fixture ----
# A net's f32 weights barely compress (Minivilles 4p: 1.3 MB raw, 1.2 MB deflated).  For such a checkpoint the fixture keeps the
# shapes and per-tensor statistics of its state_dict (`weightstats_<tag>.npz`, tools/convert_ckpt.py) and the weights are drawn from
# them with numpy's PCG64 generator, which gives the same numbers on every platform; the reference's own module is evaluated on those
# weights for the forward vectors.
def weight_stats(state_dict, seed=0):
    """state_dict (numpy arrays) -> the arrays of a weightstats_<tag>.npz: 'shape/<key>', 'stat/<key>' = (mean, std) -- of log(x)
    for BatchNorm running variances, which must stay positive --, integer tensors ('int/<key>') kept as they are, and the seed"""
    out = {'seed': np.array(seed)}
    for k, v in state_dict.items():
        v = np.asarray(v)
        if not np.issubdtype(v.dtype, np.floating):
            out['int/' + k] = v
            continue
        x = np.log(v.astype(np.float64)) if k.endswith('running_var') else v.astype(np.float64)
        out['shape/' + k] = np.array(v.shape, dtype=np.int64)
        out['stat/' + k] = np.array([x.mean(), x.std()])
    return out


def synthetic_state_dict(z):
    """the stand-in state_dict (float32 numpy arrays) of a weightstats_<tag>.npz: keys in sorted order, each tensor drawn as
    mean + std * N(0, 1) (exp of that for running variances) from one PCG64 stream"""
    files = list(z.files) if hasattr(z, 'files') else list(z)
    rng = np.random.default_rng(int(z['seed']))
    sd = {}
    for name in sorted(n[6:] for n in files if n.startswith('shape/')):
        mean, std = (float(t) for t in z['stat/' + name])
        x = mean + std * rng.standard_normal(tuple(int(s) for s in z['shape/' + name]))
        sd[name] = (np.exp(x) if name.endswith('running_var') else x).astype(np.float32)
    sd.update({n[4:]: np.asarray(z[n]) for n in files if n.startswith('int/')})
    return sd


def fixture_state_dict(golden_dir, tag):
    """(state_dict as numpy arrays, {arg: value}) of a net fixture: the shipped weights of weights_<tag>.npz, or the stand-in weights of
    weightstats_<tag>.npz for a checkpoint too large to keep"""
    import os
    path = os.path.join(golden_dir, 'weights_%s.npz' % tag)
    if os.path.exists(path):
        z = np.load(path)
        sd = {k[3:]: np.asarray(z[k]) for k in z.files if k.startswith('sd/')}
    else:
        z = np.load(os.path.join(golden_dir, 'weightstats_%s.npz' % tag))
        sd = synthetic_state_dict(z)
    return sd, {k[4:]: z[k] for k in z.files if k.startswith('arg/')}
