"""NeuralNet.predict for the engine: one batched PyTorch-ROCm forward over the leaf batch (the only MFMA work on the
path).  Replaces GenericNNetWrapper.predict / predict_client / predict_server (GenericNNetWrapper.py:94-157): instead of
N threads time-slicing one core to build an ONNX batch of N, the forest's select kernel writes all T leaves and this
module evaluates them in one pass.

SplendorV80 re-expresses the reference's nn_version == 80 network (splendor/SplendorNNet.py:262-283,397-440 and the
blocks :148-202) in plain torch -- no torchvision -- in channels-last layout [B, 7, C] so every token-axis Linear is a
plain GEMM, with BatchNorm folded into the GEMM weights (eval mode) and the Flatten permutation folded into the first
head Linear.  It loads the reference's state_dict key names unchanged (checkpoint compatibility)."""
import copy
import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as F


def _fold_bn(sd, prefix, eps=1e-5):
    g, b = sd[prefix + '.weight'], sd[prefix + '.bias']
    m, v = sd[prefix + '.running_mean'], sd[prefix + '.running_var']
    s = g / torch.sqrt(v + eps)
    return s, b - m * s


def _wide(dtype):
    """the dtype a plain-torch net folds its BatchNorms in and returns pi / v in: f32, or f64 for a float64 net (the f64 evaluation of
    a net is the reference the kernels are held to: it must not carry f32 folds or an f32 softmax)"""
    return torch.float64 if dtype == torch.float64 else torch.float32


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _pow2_scale(maxabs):
    """the exponent k of the f16 x 2 operands: maxabs * 2^k in (2^11, 2^12] (an all-zero matrix: any scale).  The kernels multiply
    their accumulators by _descale(k)"""
    return 12 - int(math.ceil(math.log2(max(float(maxabs), 1e-30))))


def _descale(k):
    return (2.0 ** -k) / 64.0


def _split_frag(m, kind, k=0):
    """zero-padded [K][N] f32 (K % 32 == 0, N % 16 == 0) -> split-precision MFMA fragments [N/16 tiles][K/32 chunks][planes][64 lanes][8]:
    frag[ct][c][p][lane][j] = plane_p[32c + 8*(lane>>4) + j][16ct + (lane&15)].  kind 'h2': the f16 hi / lo planes of m * 2^k;
    'bf16x3': the bf16 hi / mid / lo planes of m"""
    K, N = m.shape
    assert K % 32 == 0 and N % 16 == 0
    m = m.contiguous().float()
    if kind == 'h2':
        m = m * (2.0 ** k)
        hi = m.to(torch.float16)
        planes = [hi, (m - hi.float()).to(torch.float16)]
    else:
        assert kind == 'bf16x3'
        hi = m.to(torch.bfloat16)
        r1 = m - hi.float()
        mid = r1.to(torch.bfloat16)
        planes = [hi, mid, (r1 - mid.float()).to(torch.bfloat16)]
    assert bool(torch.isfinite(hi.float()).all())
    pl = torch.stack(planes).view(len(planes), K // 32, 4, 8, N // 16, 16)                # plane, chunk, g, j, tile, r
    return pl.permute(4, 1, 0, 2, 5, 3).contiguous().view(-1)                             # tile, chunk, plane, g, r, j


def _pad(t, shape):
    """t zero-padded to `shape` (f32, a fresh tensor)"""
    out = torch.zeros(shape, dtype=torch.float32, device=t.device)
    out[tuple(slice(0, n) for n in t.shape)] = t
    return out


def _frag(Wp, half_last=False):
    """zero-padded [Kp][NP] f32 -> MFMA fragment order [NP/16][Kp/16][64 lanes][4]:
    frag[nt][c][lane][j] = Wp[16c + 4*(lane>>4) + j][16nt + (lane&15)]  (FRAG in csrc/nn_kernels.hip.h).
    half_last: the last chunk holds only 8 rows of K; lane group g gets rows 16c + 2g + {0, 1} in j = 0, 1"""
    Kp, NP = Wp.shape
    assert Kp % 16 == 0 and NP % 16 == 0
    if half_last:
        last = Wp[Kp - 16:].clone()
        assert float(last[8:].abs().max()) == 0.0
        Wp = Wp.clone()
        Wp[Kp - 16:] = 0
        for g in range(4):
            Wp[Kp - 16 + 4 * g: Kp - 16 + 4 * g + 2] = last[2 * g: 2 * g + 2]
    return Wp.view(Kp // 16, 4, 4, NP // 16, 16).permute(3, 0, 1, 4, 2).contiguous().view(-1)


def _r16(n):
    return (n + 15) // 16 * 16


def _flat_rows(Wf, L, stride):
    """a flatten -> Linear weight [L*c][N] (row k = l*c + ch) re-indexed to the kernels' token tile of row stride `stride`:
    [L*stride][N], row k = l*stride + ch (the pad rows zero)"""
    c = Wf.shape[0] // L
    return _pad(Wf.view(L, c, -1), (L, stride, Wf.shape[1])).view(L * stride, -1)


class _TorchNet:
    """NeuralNet-style entry points of the plain-torch nets: a subclass has __init__(state_dict, ..., device=...), device and
    forward(boards, valids bool) -> (pi, v)."""

    @classmethod
    def from_npz(cls, path, **kw):
        z = np.load(path)
        return cls({k[3:]: z[k] for k in z.files if k.startswith('sd/')}, **kw)

    # NeuralNet.predict-compatible entry points
    def predict_batch(self, boards, valids):
        return self.forward(boards, valids)

    def predict(self, board, valid_actions):
        b = torch.from_numpy(np.ascontiguousarray(board, dtype=np.int8))[None].to(self.device)
        va = torch.from_numpy(np.asarray(valid_actions).astype(np.bool_))[None].to(self.device)
        pi, v = self.forward(b, va)
        return pi[0].cpu().numpy(), v[0].cpu().numpy()


class _EngineNet:
    """An engine evaluator: a net's weights packed for one of the engine's one-launch forward kernels, with static pi [maxB, A] /
    v [maxB, P] output buffers (the engine's rounds are captured into HIP graphs with them).  A subclass sets _lib, device, A, P,
    S (the board width in bytes) and ptrs (the weight pointer table), and either names the C entry point in _FN with the integers
    it takes before B in _ints(), or overrides _launch (boards, valids: device pointers)."""
    _FN = None

    def _ints(self):
        raise NotImplementedError

    def _alloc(self, B):
        self.maxB = B
        self.pi = torch.empty((B, self.A), dtype=torch.float32, device=self.device)
        self.v = torch.empty((B, self.P), dtype=torch.float32, device=self.device)

    def clone_buffers(self):
        """a second evaluator sharing the (read-only) weights but with its own activation buffers (concurrent streams)"""
        other = copy.copy(self)
        other._alloc(self.maxB)
        return other

    @staticmethod
    def _stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @torch.no_grad()
    def forward(self, boards, valids):
        B = boards.shape[0]
        if B > self.maxB:
            self._alloc(B)
        boards = boards.reshape(B, -1)
        assert boards.dtype == torch.int8 and boards.is_contiguous() and boards.is_cuda and boards.shape[1] == self.S
        valids = (valids if valids.dtype == torch.uint8 else valids.to(torch.uint8)).contiguous()
        assert valids.shape == (B, self.A) and valids.is_cuda
        self._launch(_ptr(boards), _ptr(valids), B, self._stream())
        return self.pi[:B], self.v[:B]

    def _launch(self, boards, valids, B, stream):
        self._lib.check(getattr(self._lib.lib(), self._FN)(boards, valids, self.ptrs, *self._ints(), B, _ptr(self.pi), _ptr(self.v), stream))

    def predict_batch(self, boards, valids):
        return self.forward(boards, valids)

    def predict(self, board, valid_actions):
        b = torch.as_tensor(np.asarray(board, dtype=np.int8)).reshape(1, -1).to(self.device)
        va = torch.as_tensor(np.asarray(valid_actions).astype(np.uint8)).reshape(1, -1).to(self.device)
        pi, v = self.forward(b, va)
        return pi[0].cpu().numpy(), v[0].cpu().numpy()


class _Block:
    """InvertedResidual1d (SplendorNNet.py:189-202) with folded BN; activations: ReLU or Hardswish; SE avg/max."""

    def __init__(self, sd, prefix, use_hs, setype):
        self.use_hs, self.setype = use_hs, setype
        s, b = _fold_bn(sd, prefix + '.expand.norm')
        self.We = (sd[prefix + '.expand.linear.weight'] * s[:, None]).t().contiguous()      # [Cin, Cexp]
        self.be = b
        s, b = _fold_bn(sd, prefix + '.depthwise.norm')
        self.Wd = sd[prefix + '.depthwise.linear.weight'].contiguous()                      # [7, 7] (out, in)
        self.sd, self.bd = s, b                                                             # per channel
        self.W1 = sd[prefix + '.se.fc1.weight'].t().contiguous()
        self.b1 = sd[prefix + '.se.fc1.bias']
        self.W2 = sd[prefix + '.se.fc2.weight'].t().contiguous()
        self.b2 = sd[prefix + '.se.fc2.bias']
        s, b = _fold_bn(sd, prefix + '.project.norm')
        self.Wp = (sd[prefix + '.project.linear.weight'] * s[:, None]).t().contiguous()     # [Cexp, Cout]
        self.bp = b

    def tensors(self):
        return ['We', 'be', 'Wd', 'sd', 'bd', 'W1', 'b1', 'W2', 'b2', 'Wp', 'bp']

    def act(self, x):
        return F.hardswish(x) if self.use_hs else F.relu(x)

    def __call__(self, x):                      # x: [B, L, C]
        h = self.act(torch.matmul(x, self.We) + self.be)                       # expand  [B,7,Cexp]
        h = torch.matmul(self.Wd.to(h.dtype), h) * self.sd + self.bd           # depthwise Linear(7->7) over L, then BN
        h = self.act(h)
        pooled = h.mean(dim=1) if self.setype == 'avg' else h.amax(dim=1)      # SE squeeze over L  [B,Cexp]
        sc = F.hardsigmoid(torch.addmm(self.b2, F.relu(torch.addmm(self.b1, pooled, self.W1)), self.W2))
        h = h * sc[:, None, :]
        out = torch.matmul(h, self.Wp) + self.bp                               # project (+BN)
        return out + x if self.Wp.shape[1] == x.shape[-1] else out             # use_res_connect: in == out channels


class SplendorV80(_TorchNet):
    """forward(board int8/float [B,56,7], valid bool [B,81]) -> (pi probabilities f32 [B,81], v f32 [B,P])."""

    def __init__(self, state_dict, num_players=2, device='cuda:0', dtype=torch.float32):
        sd = {k: torch.as_tensor(v).to(_wide(dtype)) for k, v in state_dict.items()}
        self.P = num_players
        self.nb_vect = 32 + 10 * num_players + num_players * num_players
        self.A = 81
        s, b = _fold_bn(sd, 'first_layer.norm')
        self.W0 = (sd['first_layer.linear.weight'] * s[:, None]).t().contiguous()
        self.b0 = b
        self.trunk = _Block(sd, 'trunk.0', False, 'avg')
        self.head_pi = _Block(sd, 'output_layers_PI.0', True, 'max')
        self.head_v = _Block(sd, 'output_layers_V.0', True, 'max')
        C = self.nb_vect

        def perm(w):   # reference flattens [B, C, 7] (index c*7+l); ours is [B, 7, C] (index l*C+c)
            return w.view(w.shape[0], C, 7).permute(0, 2, 1).reshape(w.shape[0], 7 * C).t().contiguous()
        self.Wpi1, self.bpi1 = perm(sd['output_layers_PI.2.weight']), sd['output_layers_PI.2.bias']
        self.Wpi2, self.bpi2 = sd['output_layers_PI.4.weight'].t().contiguous(), sd['output_layers_PI.4.bias']
        self.Wv1, self.bv1 = perm(sd['output_layers_V.2.weight']), sd['output_layers_V.2.bias']
        self.Wv2, self.bv2 = sd['output_layers_V.4.weight'].t().contiguous(), sd['output_layers_V.4.bias']
        self.to(device, dtype)

    def to(self, device, dtype=torch.float32):
        self.device, self.dtype = torch.device(device), dtype
        for name in ['W0', 'b0', 'Wpi1', 'bpi1', 'Wpi2', 'bpi2', 'Wv1', 'bv1', 'Wv2', 'bv2']:
            setattr(self, name, getattr(self, name).to(self.device, dtype))
        for blk in (self.trunk, self.head_pi, self.head_v):
            for name in blk.tensors():
                setattr(blk, name, getattr(blk, name).to(self.device, dtype))
        return self

    @classmethod
    def random_init(cls, num_players=2, seed=0, **kw):
        """random weights of the V80 architecture (for runs without a checkpoint)"""
        return cls(cls.random_state_dict(num_players, seed), num_players=num_players, **kw)

    @staticmethod
    def random_state_dict(num_players=2, seed=0):
        g = torch.Generator().manual_seed(seed)
        C, E, Q = 32 + 10 * num_players + num_players * num_players, 0, 0
        E = 3 * C
        Q = max(8, int(E // 4 + 4) // 8 * 8)
        sd = {}

        def lin(name, o, i, bias=True):
            sd[name + '.weight'] = (torch.rand(o, i, generator=g) * 2 - 1) * (6.0 / i) ** 0.5
            if bias:
                sd[name + '.bias'] = torch.zeros(o)

        def bn(name, c):
            sd[name + '.weight'], sd[name + '.bias'] = torch.ones(c), torch.zeros(c)
            sd[name + '.running_mean'], sd[name + '.running_var'] = torch.zeros(c), torch.ones(c)

        def block(p):
            lin(p + '.expand.linear', E, C, False); bn(p + '.expand.norm', E)
            lin(p + '.depthwise.linear', 7, 7, False); bn(p + '.depthwise.norm', E)
            lin(p + '.se.fc1', Q, E); lin(p + '.se.fc2', E, Q)
            lin(p + '.project.linear', C, E, False); bn(p + '.project.norm', C)
        lin('first_layer.linear', C, C, False); bn('first_layer.norm', C)
        block('trunk.0'); block('output_layers_PI.0'); block('output_layers_V.0')
        lin('output_layers_PI.2', 81, 7 * C); lin('output_layers_PI.4', 81, 81)
        lin('output_layers_V.2', num_players, 7 * C); lin('output_layers_V.4', num_players, num_players)
        return sd

    @torch.no_grad()
    def forward(self, boards, valids):
        B = boards.shape[0]
        x = boards.reshape(B, self.nb_vect, 7).to(self.dtype).transpose(1, 2)                 # [B,7,C] view
        x = torch.matmul(x, self.W0) + self.b0                                                 # first_layer (+BN)
        x = self.trunk(x)
        hp = self.head_pi(x).reshape(B, -1)
        logits = torch.addmm(self.bpi2, F.relu(torch.addmm(self.bpi1, hp, self.Wpi1)), self.Wpi2).to(_wide(self.dtype))
        hv = self.head_v(x).reshape(B, -1)
        v = torch.tanh(torch.addmm(self.bv2, F.relu(torch.addmm(self.bv1, hv, self.Wv1)), self.Wv2).to(_wide(self.dtype)))
        logits = torch.where(valids.bool(), logits, torch.full_like(logits, -1e8))            # SplendorNNet.py:404
        pi = torch.softmax(logits, dim=1)              # exp(log_softmax) of GenericNNetWrapper.py:107,119
        return pi.contiguous(), v.contiguous()


class SplendorV80Hip(_EngineNet, SplendorV80):
    """Same network, same weights, evaluated by one launch of the engine's own gfx950 kernels instead of ~70 torch ops per leaf batch:
    first layer, the three InvertedResidual1d blocks and both head tails on a 16-sample tile that never leaves LDS (azg_nn_v80_forward*
    in include/azg.h).  The weights are packed once, as three 43-slot pointer tables (f32, bf16 x 3 and f16 x 2 operands); forward and predict are
    _EngineNet's (bool or uint8 valids), the torch model underneath is SplendorV80's."""
    S = 56 * 7

    def __init__(self, state_dict, num_players=2, device='cuda:0', max_batch=4096, split=True, h2=None):
        """h2 (default for the 2-player geometry): the forward on fp16 hi+lo split operands with token-major tiles
        (azg_nn_v80_forward_h2, csrc/nn_v80_h2.hip.h; same 1e-5 contract).  Otherwise split: the tile the blocks read is kept as
        three bf16 planes and the expand GEMMs run on bf16 x 3 operands (azg_nn_v80_forward_split); False = f32 MFMAs throughout"""
        super().__init__(state_dict, num_players=num_players, device=device, dtype=torch.float32)
        from . import _lib
        self._lib = _lib
        self.split = bool(split)
        self.h2 = (self.nb_vect == 56) if h2 is None else bool(h2)
        self.C = self.nb_vect
        self.fused_net = True          # the one-launch forward is the only form there is (forest.py's matcher reads this)
        self._net_ptrs()
        self._h2_ptrs()
        self._alloc(max_batch)

    def _net_ptrs(self):
        """device pointer tables of azg_nn_v80_forward / _split (include/azg.h): first layer, 3 blocks, head Linears re-indexed to the
        in-LDS flatten k = l*60 + c; _split differs in the three expand matrices only"""
        blocks = (self.trunk, self.head_pi, self.head_v)
        assert [(b.use_hs, b.setype) for b in blocks] == [(False, 'avg'), (True, 'max'), (True, 'max')]
        assert self.C == 56 and self.A == 81
        pad = _pad
        keep = [_frag(pad(self.W0, (64, 64)), True), pad(self.b0, (64,))]
        for blk in blocks:
            keep += [_frag(pad(blk.We, (64, 176)), True), pad(blk.be, (176,)), blk.Wd.contiguous(), blk.sd.contiguous(), blk.bd.contiguous(),
                     _frag(pad(blk.W1, (176, 48)), True), pad(blk.b1, (48,)), _frag(pad(blk.W2, (48, 176))), pad(blk.b2, (176,)),
                     _frag(pad(blk.Wp, (176, 64)), True), pad(blk.bp, (64,))]
        keep += [_frag(pad(_flat_rows(self.Wpi1, 7, 60), (432, 96))), pad(self.bpi1, (96,)), _frag(pad(self.Wpi2, (96, 96))),
                 pad(self.bpi2, (96,)), _frag(pad(_flat_rows(self.Wv1, 7, 60), (432, 16))), pad(self.bv1, (16,)), self.Wv2.contiguous(),
                 self.bv2.contiguous()]
        assert len(keep) == 43
        self._net_keep = keep
        self.net_ptrs = (C.c_void_p * 43)(*[t.data_ptr() for t in keep])
        keep = list(keep)
        for bi, blk in enumerate(blocks):
            keep[2 + 11 * bi] = _split_frag(pad(blk.We, (64, 176)), 'bf16x3')     # K 56 -> 64 zero padded
        self._net_keep_split = keep
        self.net_ptrs_split = (C.c_void_p * 43)(*[t.data_ptr() for t in keep])

    def _h2_ptrs(self):
        """pointer table + descale factors of azg_nn_v80_forward_h2 (include/azg.h): every matrix zero padded to K % 32 == 0,
        N % 16 == 0, scaled by 2^k (max |w| * 2^k in (2^11, 2^12]) and split into f16 hi / lo fragments"""
        f, pad = torch.float32, _pad

        def frag(W, K, N):
            k = _pow2_scale(W.abs().max())
            return _split_frag(pad(W, (K, N)), 'h2', k), _descale(k)
        keep, desc = [], []
        t, s = frag(self.W0, 64, 64)
        keep += [t, pad(self.b0, (64,))]
        desc.append(s)
        for blk in (self.trunk, self.head_pi, self.head_v):
            we, se = frag(blk.We, 64, 176)
            w1, s1 = frag(blk.W1, 192, 48)
            w2, s2 = frag(blk.W2, 64, 176)
            wp, sp = frag(blk.Wp, 192, 64)
            keep += [we, pad(blk.be, (176,)), (blk.Wd / 6.0 if blk.use_hs else blk.Wd).contiguous().to(f), pad(blk.sd, (176,)), pad(blk.bd, (176,)), w1, pad(blk.b1, (48,)),
                     w2, pad(blk.b2, (176,)), wp, pad(blk.bp, (64,))]
            desc += [se, s1, s2, sp]
        wpi1, spi1 = frag(_flat_rows(self.Wpi1, 7, 64), 448, 96)            # row k = l*64 + c
        wpi2, spi2 = frag(self.Wpi2, 96, 96)
        wv1, sv1 = frag(_flat_rows(self.Wv1, 7, 64), 448, 16)
        keep += [wpi1, pad(self.bpi1, (96,)), wpi2, pad(self.bpi2, (96,)), wv1, pad(self.bv1, (16,)), self.Wv2.contiguous(), self.bv2.contiguous()]
        desc += [spi1, spi2, sv1]
        assert len(keep) == 43 and len(desc) == 16
        self._net_keep_h2 = keep
        self.net_ptrs_h2 = (C.c_void_p * 43)(*[t.data_ptr() for t in keep])
        self.descale_h2 = (C.c_float * 16)(*desc)

    def _launch(self, boards, valids, B, stream):
        L = self._lib.lib()
        if self.h2:
            self._lib.check(L.azg_nn_v80_forward_h2(boards, valids, self.net_ptrs_h2, self.descale_h2, B, self.P, _ptr(self.pi), _ptr(self.v), stream))
            return
        fwd, ptrs = (L.azg_nn_v80_forward_split, self.net_ptrs_split) if self.split else (L.azg_nn_v80_forward, self.net_ptrs)
        self._lib.check(fwd(boards, valids, ptrs, B, self.P, _ptr(self.pi), _ptr(self.v), stream))


class AzulV84(SplendorV80):
    """azul/AzulNNet.py nn_version == 84 (:91-113,130-142): same building blocks on a [B, 23, 6] board -- trunk block
    23->115->23, policy head block 23->115->46 (no residual) + Linear(276,180)+ReLU+Linear, value head block 23->46->23."""

    def __init__(self, state_dict, num_players=2, device='cuda:0', dtype=torch.float32):
        sd = {k: torch.as_tensor(v).to(_wide(dtype)) for k, v in state_dict.items()}
        self.P = num_players
        self.nb_vect, self.L, self.A = 23, 6, 180
        s, b = _fold_bn(sd, 'first_layer.norm')
        self.W0 = (sd['first_layer.linear.weight'] * s[:, None]).t().contiguous()
        self.b0 = b
        self.trunk = _Block(sd, 'trunk.0', False, 'avg')
        self.head_pi = _Block(sd, 'output_layers_PI.0', True, 'avg')
        self.head_v = _Block(sd, 'output_layers_V.0', True, 'avg')
        L = self.L

        def perm(w, C):   # reference flattens [B, C, L] (index c*L+l); ours is [B, L, C] (index l*C+c)
            return w.view(w.shape[0], C, L).permute(0, 2, 1).reshape(w.shape[0], L * C).t().contiguous()
        self.Wpi1, self.bpi1 = perm(sd['output_layers_PI.2.weight'], 46), sd['output_layers_PI.2.bias']
        self.Wpi2, self.bpi2 = sd['output_layers_PI.4.weight'].t().contiguous(), sd['output_layers_PI.4.bias']
        self.Wv1, self.bv1 = perm(sd['output_layers_V.2.weight'], 23), sd['output_layers_V.2.bias']
        self.Wv2, self.bv2 = sd['output_layers_V.4.weight'].t().contiguous(), sd['output_layers_V.4.bias']
        self.to(device, dtype)

    @torch.no_grad()
    def forward(self, boards, valids):
        B = boards.shape[0]
        x = boards.reshape(B, self.nb_vect, self.L).to(self.dtype).transpose(1, 2)
        x = torch.matmul(x, self.W0) + self.b0
        x = self.trunk(x)
        hp = self.head_pi(x).reshape(B, -1)
        logits = torch.addmm(self.bpi2, F.relu(torch.addmm(self.bpi1, hp, self.Wpi1)), self.Wpi2).to(_wide(self.dtype))
        hv = self.head_v(x).reshape(B, -1)
        v = torch.tanh(torch.addmm(self.bv2, F.relu(torch.addmm(self.bv1, hv, self.Wv1)), self.Wv2).to(_wide(self.dtype)))
        logits = torch.where(valids.bool(), logits, torch.full_like(logits, -1e8))
        return torch.softmax(logits, dim=1).contiguous(), v.contiguous()


class MobileNet1d(AzulV84):
    """Any net of the reference's one-trunk-block MobileNetV3-1d family, geometry read off the state_dict: first_layer, ONE trunk block
    (ReLU, mean squeeze), one policy-head and one value-head block (Hardswish, `head_se` squeeze), Flatten + Linear + ReLU + Linear heads.
    The shipped nets of two more games are of this shape at every shipped player count (their checkpoints load unchanged):
      minivilles/MinivillesNNet.py:101-123 nn_version 82 -- [B, 58, 2] board (2 players), blocks 58 -> 174 -> 58, heads Linear(116, 21) / (116, 2);
                                                           C = 18 + 20 P and E = 3C for 3 / 4 players ([B, 78 | 98, 2])
      thelittleprince/TLPNNet.py:175-196 nn_version 83   -- [B, 55, 15] board (3 players), blocks 55 -> 82 -> 55, heads Linear(825, 9) / (825, 3);
                                                           C = 1 + 18 P and E = int(1.5 C) for 4 / 5 players ([B, 73 | 91, 15])
    (TLP nn_version 80 / 82 differ in the expansion factor only and load the same way.)"""

    def __init__(self, state_dict, num_players=None, head_se='max', device='cuda:0', dtype=torch.float32):
        sd = {k: torch.as_tensor(v).to(_wide(dtype)) for k, v in state_dict.items()}
        self.nb_vect = int(sd['first_layer.linear.weight'].shape[0])
        self.L = L = int(sd['trunk.0.depthwise.linear.weight'].shape[0])
        self.A = int(sd['output_layers_PI.4.weight'].shape[0])
        self.P = int(sd['output_layers_V.4.weight'].shape[0])
        assert num_players in (None, self.P)
        s, b = _fold_bn(sd, 'first_layer.norm')
        self.W0 = (sd['first_layer.linear.weight'] * s[:, None]).t().contiguous()
        self.b0 = b
        self.trunk = _Block(sd, 'trunk.0', False, 'avg')
        self.head_pi = _Block(sd, 'output_layers_PI.0', True, head_se)
        self.head_v = _Block(sd, 'output_layers_V.0', True, head_se)

        def perm(w, C):   # reference flattens [B, C, L] (index c*L+l); ours is [B, L, C] (index l*C+c)
            return w.view(w.shape[0], C, L).permute(0, 2, 1).reshape(w.shape[0], L * C).t().contiguous()
        self.Wpi1, self.bpi1 = perm(sd['output_layers_PI.2.weight'], self.head_pi.Wp.shape[1]), sd['output_layers_PI.2.bias']
        self.Wpi2, self.bpi2 = sd['output_layers_PI.4.weight'].t().contiguous(), sd['output_layers_PI.4.bias']
        self.Wv1, self.bv1 = perm(sd['output_layers_V.2.weight'], self.head_v.Wp.shape[1]), sd['output_layers_V.2.bias']
        self.Wv2, self.bv2 = sd['output_layers_V.4.weight'].t().contiguous(), sd['output_layers_V.4.bias']
        self.to(device, dtype)


class MinivillesV82(MobileNet1d):
    """minivilles/MinivillesNNet.py nn_version == 82 (:101-123,166-172), the net of all shipped player counts
    (minivilles/pretrained_{2,3,4}players.pt: [58 | 78 | 98][2] boards)"""


class TLPV83(MobileNet1d):
    """thelittleprince/TLPNNet.py nn_version == 83 (:175-196,211-217), the net of all shipped player counts
    (thelittleprince/pretrained_{3,4,5}players.pt: [55 | 73 | 91][15] boards)"""


# (tokens L, channels C) -> AZG_NET_* geometry id of azg_nn_mb1d_forward (include/azg.h)
MB1D_GEOMETRY = {(7, 56): 0, (7, 71): 1, (7, 88): 2, (6, 23): 3, (2, 58): 4, (15, 55): 5,
                 (2, 78): 6, (2, 98): 7, (15, 73): 8, (15, 91): 9}


class MobileNet1dHip(_EngineNet):
    """The MobileNetV3-1d policy/value nets of any geometry in MB1D_GEOMETRY (Splendor V80 for 2-4 players: C = 32 + 10n + n^2 channels x 7
    tokens; Azul V84: 23 channels x 6 tokens, AzulNNet.py:91-113; Minivilles V82; The Little Prince V83) evaluated by one launch of the
    engine's gfx950 kernel (azg_nn_mb1d_forward / _h2, csrc/nn_mb1d.hip.h) instead of ~65 torch ops per leaf batch.  Wraps a SplendorV80 /
    AzulV84 / MobileNet1d instance (folded-BN fp32 weights); matrices are zero-padded to multiples of 16 (K to 32 for the f16 x 2
    operands) and stored in MFMA fragment order, which leaves the results unchanged."""

    def __init__(self, base, max_batch=4096, fused=True, h2=True):
        """h2 (default): the GEMM phases on f16 x 2 split-precision operands (azg_nn_mb1d_forward_h2); False = f32 MFMAs throughout"""
        from . import _lib
        self._lib = _lib
        self.base = base
        self.h2 = h2
        self.device = base.device
        self.P, self.A, self.C = base.P, base.A, base.nb_vect
        self.L = getattr(base, 'L', 7)
        self.nb_vect = base.nb_vect
        self.S = self.C * self.L
        self.geometry = MB1D_GEOMETRY.get((self.L, self.C))
        if not fused or self.geometry is None:
            raise ValueError('MobileNet1dHip: the one-launch kernels are the only form (fused=True, a geometry of MB1D_GEOMETRY); got '
                             'fused=%r, L=%d C=%d' % (fused, self.L, self.C))
        self.fused = True              # the one-launch forward is the only form there is (tests and tools read this)
        assert base.dtype == torch.float32 and self.device.type == 'cuda'
        self._pack()
        self._alloc(max_batch)

    def _pack(self):
        """the 43 weight pointers of azg_nn_mb1d_forward: matrices zero-padded to multiples of 16 and stored in MFMA
        fragment order, vectors zero-padded to multiples of 16"""
        base, L, r16 = self.base, self.L, _r16
        padv = lambda v, n: _pad(v, (n,))  # noqa: E731
        fw = lambda W: _frag(_pad(W, (r16(W.shape[0]), r16(W.shape[1]))))  # noqa: E731
        keep = [fw(base.W0), padv(base.b0, r16(self.C))]
        for blk in (base.trunk, base.head_pi, base.head_v):
            E, Q, co = blk.We.shape[1], blk.W1.shape[1], blk.Wp.shape[1]
            keep += [fw(blk.We), padv(blk.be, r16(E)), blk.Wd.contiguous(), padv(blk.sd, r16(E)), padv(blk.bd, r16(E)),
                     fw(blk.W1), padv(blk.b1, r16(Q)), fw(blk.W2), padv(blk.b2, r16(E)), fw(blk.Wp), padv(blk.bp, r16(co))]
        OS = r16(max(self.C, base.head_pi.Wp.shape[1])) + 4             # row stride of the kernel's output tile: row k = l*OS + c
        wpi1, wv1 = _flat_rows(base.Wpi1, L, OS), _flat_rows(base.Wv1, L, OS)
        keep += [fw(wpi1), padv(base.bpi1, r16(self.A)), fw(base.Wpi2), padv(base.bpi2, r16(self.A)),
                 fw(wv1), padv(base.bv1, 16), base.Wv2.contiguous(), base.bv2.contiguous()]
        assert len(keep) == 43
        self._fused_keep = keep
        self.fused_ptrs = (C.c_void_p * 43)(*[t.data_ptr() for t in keep])
        # azg_nn_mb1d_forward_h2: the same table with the matrices as f16 x 2 fragments (K padded to multiples of 32)
        desc = []

        def fh(W):
            k = _pow2_scale(W.abs().max())
            desc.append(_descale(k))
            return _split_frag(_pad(W, ((r16(W.shape[0]) + 31) // 32 * 32, r16(W.shape[1]))), 'h2', k)
        k2 = list(keep)
        k2[0] = fh(base.W0)
        for b, blk in enumerate((base.trunk, base.head_pi, base.head_v)):
            o = 2 + 11 * b
            k2[o], k2[o + 5], k2[o + 7], k2[o + 9] = fh(blk.We), fh(blk.W1), fh(blk.W2), fh(blk.Wp)
        k2[35], k2[37], k2[39] = fh(wpi1), fh(base.Wpi2), fh(wv1)
        assert len(desc) == 16
        self._fused_keep_h2 = k2
        self.fused_ptrs_h2 = (C.c_void_p * 43)(*[t.data_ptr() for t in k2])
        self.descale_h2 = (C.c_float * 16)(*desc)

    def _launch(self, boards, valids, B, stream):
        L = self._lib.lib()
        if self.h2:
            self._lib.check(L.azg_nn_mb1d_forward_h2(self.geometry, boards, valids, self.fused_ptrs_h2, self.descale_h2, B, _ptr(self.pi), _ptr(self.v), stream))
        else:
            self._lib.check(L.azg_nn_mb1d_forward(self.geometry, boards, valids, self.fused_ptrs, B, _ptr(self.pi), _ptr(self.v), stream))


class SantoriniV89(_TorchNet):
    """santorini/SantoriniNNet.py nn_version 88/89 (:194-219,273-281; SimpleResBlock :71-84, SimpleHead :17-40): the 2
    spatial planes (workers, levels) of the (5,5,3) board -> conv3x3(2->64)+BN+ReLU -> 5 residual blocks -> 1x1-conv heads.
    BatchNorm folded into the convolutions (eval mode); plain torch ops (MIOpen / hipBLASLt)."""

    def __init__(self, state_dict, num_players=2, device='cuda:0', dtype=torch.float32):
        sd = {k: torch.as_tensor(v).to(_wide(dtype)) for k, v in state_dict.items()}
        self.P, self.A = num_players, sd['head_PI.fc.weight'].shape[0]

        def conv_bn(conv, bn):
            s, b = _fold_bn(sd, bn)
            return (sd[conv + '.weight'] * s[:, None, None, None]).contiguous(), b
        self.c0 = conv_bn('first_layer.0', 'first_layer.1')
        self.blocks = []
        i = 0
        while 'trunk.%d.conv1.weight' % i in sd:
            self.blocks.append((conv_bn('trunk.%d.conv1' % i, 'trunk.%d.bn1' % i),
                                conv_bn('trunk.%d.conv2' % i, 'trunk.%d.bn2' % i)))
            i += 1
        self.hp = conv_bn('head_PI.conv1x1', 'head_PI.bn')
        self.hv = conv_bn('head_V.conv1x1', 'head_V.bn')
        self.fc_pi = (sd['head_PI.fc.weight'].t().contiguous(), sd['head_PI.fc.bias'])
        self.fc_v1 = (sd['head_V.fc1.weight'].t().contiguous(), sd['head_V.fc1.bias'])
        self.fc_v2 = (sd['head_V.fc2.weight'].t().contiguous(), sd['head_V.fc2.bias'])
        self.to(device, dtype)

    def to(self, device, dtype=torch.float32):
        self.device, self.dtype = torch.device(device), dtype
        mv = lambda pr: tuple(t.to(self.device, dtype) for t in pr)  # noqa: E731
        self.c0, self.hp, self.hv = mv(self.c0), mv(self.hp), mv(self.hv)
        self.blocks = [(mv(a), mv(b)) for a, b in self.blocks]
        self.fc_pi, self.fc_v1, self.fc_v2 = mv(self.fc_pi), mv(self.fc_v1), mv(self.fc_v2)
        return self

    @torch.no_grad()
    def forward(self, boards, valids):
        B = boards.shape[0]
        x = boards.reshape(B, 5, 5, 3).to(self.dtype).permute(0, 3, 1, 2)[:, :2].contiguous()
        x = F.relu(F.conv2d(x, self.c0[0], self.c0[1], padding=1))
        for (w1, b1), (w2, b2) in self.blocks:
            y = F.relu(F.conv2d(x, w1, b1, padding=1))
            x = F.relu(F.conv2d(y, w2, b2, padding=1) + x)
        hp = F.relu(F.conv2d(x, self.hp[0], self.hp[1])).flatten(1)
        logits = torch.addmm(self.fc_pi[1], hp, self.fc_pi[0]).to(_wide(self.dtype))
        hv = F.relu(F.conv2d(x, self.hv[0], self.hv[1])).flatten(1)
        v = torch.tanh(torch.addmm(self.fc_v2[1], F.relu(torch.addmm(self.fc_v1[1], hv, self.fc_v1[0])), self.fc_v2[0]).to(_wide(self.dtype)))
        logits = torch.where(valids.bool(), logits, torch.full_like(logits, -1e8))
        return torch.softmax(logits, dim=1).contiguous(), v.contiguous()


class SantoriniV89Hip(_EngineNet):
    """SantoriniV89 (no-gods geometry: 5 residual blocks, A = 162) evaluated by the engine's one-launch implicit-GEMM kernel
    (azg_nn_conv5_forward, csrc/nn_conv5x5.hip.h) instead of 11 MIOpen convolutions + glue ops.  Wraps a SantoriniV89."""
    S = 75

    def __init__(self, base, max_batch=4096, split=True, h2=True):
        """h2 (default): the trunk convolutions on f16 x 2 split-precision operands (azg_nn_conv5_forward_h2: three f16 MFMAs per
        product, 22-bit operands, same 1e-5 contract).  Otherwise split: bf16 x 3 (azg_nn_conv5_forward_split, six MFMAs per
        product); False = the f32-MFMA kernel"""
        from . import _lib
        self._lib, self.base, self.device, self.split, self.h2 = _lib, base, base.device, bool(split), bool(h2)
        self.P, self.A = base.P, base.A
        assert base.dtype == torch.float32 and self.device.type == 'cuda' and len(base.blocks) == 5 and self.A == 162 and self.P == 2
        frag = _frag
        d = self.device

        def conv_rows(w):                  # [co][ci][3][3] -> [K = tap*64 + ci][co]
            co, ci = w.shape[0], w.shape[1]
            return w.permute(2, 3, 1, 0).reshape(9 * ci, co)

        def conv_split(w):                 # -> [4 ct][18 chunks][3 planes hi, mid, lo][64 lanes][8] bf16
            return _split_frag(conv_rows(w), 'bf16x3')

        def conv_mat(w, cin_pad):          # [co][ci][3][3] -> [tap*cin_pad + ci][co], fragment order
            co, ci = w.shape[0], w.shape[1]
            m = torch.zeros((9, cin_pad, co), dtype=torch.float32, device=d)
            m[:, :ci] = w.permute(2, 3, 1, 0).reshape(9, ci, co)
            return frag(m.reshape(9 * cin_pad, co).contiguous())
        convs = [c for blk in base.blocks for c in blk]
        k2 = _pow2_scale(max(float(w.abs().max()) for w, _ in convs))       # one power-of-two scale for the whole trunk
        self.descale = _descale(k2)

        def conv_h2(w):                    # -> [4 ct][18 chunks][2 planes hi, lo][64 lanes][8] f16 of W * 2^k
            return _split_frag(conv_rows(w), 'h2', k2)
        keep = [conv_mat(base.c0[0], 16), base.c0[1].contiguous(),
                torch.cat([(conv_h2(w) if self.h2 else conv_split(w) if self.split else conv_mat(w, 64)) for w, _ in convs]).contiguous(),
                torch.cat([b for _, b in convs]).contiguous(),
                base.hp[0].reshape(2, 64).t().contiguous(), base.hp[1].contiguous(), base.fc_pi[0].contiguous(), base.fc_pi[1].contiguous(),
                base.hv[0].reshape(64).contiguous(), base.hv[1].contiguous(), base.fc_v1[0].contiguous(), base.fc_v1[1].contiguous(),
                base.fc_v2[0].contiguous(), base.fc_v2[1].contiguous()]
        self._keep = keep
        self.ptrs = (C.c_void_p * 14)(*[t.data_ptr() for t in keep])
        self._alloc(max_batch)

    def _launch(self, boards, valids, B, stream):
        L = self._lib.lib()
        if self.h2:
            self._lib.check(L.azg_nn_conv5_forward_h2(boards, valids, self.ptrs, self.descale, 5, self.A, self.P, B, _ptr(self.pi), _ptr(self.v),
                                                      stream))
            return
        fwd = L.azg_nn_conv5_forward_split if self.split else L.azg_nn_conv5_forward
        self._lib.check(fwd(boards, valids, self.ptrs, 5, self.A, self.P, B, _ptr(self.pi), _ptr(self.v), stream))


class SantoriniV78(SantoriniV89):
    """santorini/SantoriniNNet.py nn_version 78 (:167-192,264-271; HeadWithMeta :42-69) -- the with-gods net of
    pretrained_withgods.pt: conv3x3(2->64, no BN) -> 10 torchvision MobileNetV3 InvertedResidual blocks (1x1 expand
    64->192 + BN + ReLU, depthwise 3x3 + BN + ReLU, 1x1 project + BN, residual; no SE) -> 1x1-conv heads whose flattened
    features are concatenated with a 32-wide embedding of the gods/metadata plane (Linear(25,32)+ReLU).  BatchNorm
    (eps 1e-5) folded into the convolutions; plain torch ops."""

    def __init__(self, state_dict, num_players=2, device='cuda:0', dtype=torch.float32):
        sd = {k: torch.as_tensor(v).to(_wide(dtype)) for k, v in state_dict.items()}
        self.P, self.A = num_players, sd['head_PI.fc.weight'].shape[0]

        def conv_bn(conv, bn):
            s, b = _fold_bn(sd, bn)
            return (sd[conv + '.weight'] * s[:, None, None, None]).contiguous(), b
        self.c0 = (sd['first_layer.weight'].contiguous(), torch.zeros(sd['first_layer.weight'].shape[0]))
        self.blocks = []
        i = 0
        while 'trunk.%d.block.0.0.weight' % i in sd:
            self.blocks.append(tuple(conv_bn('trunk.%d.block.%d.0' % (i, j), 'trunk.%d.block.%d.1' % (i, j)) for j in range(3)))
            i += 1
        self.hp = conv_bn('head_PI.conv1x1', 'head_PI.bn')
        self.hv = conv_bn('head_V.conv1x1', 'head_V.bn')
        self.meta = (sd['meta_fc.1.weight'].t().contiguous(), sd['meta_fc.1.bias'])
        self.fc_pi = (sd['head_PI.fc.weight'].t().contiguous(), sd['head_PI.fc.bias'])
        self.fc_v1 = (sd['head_V.fc1.weight'].t().contiguous(), sd['head_V.fc1.bias'])
        self.fc_v2 = (sd['head_V.fc2.weight'].t().contiguous(), sd['head_V.fc2.bias'])
        self.to(device, dtype)

    def to(self, device, dtype=torch.float32):
        self.device, self.dtype = torch.device(device), dtype
        mv = lambda pr: tuple(t.to(self.device, dtype) for t in pr)  # noqa: E731
        self.c0, self.hp, self.hv, self.meta = mv(self.c0), mv(self.hp), mv(self.hv), mv(self.meta)
        self.blocks = [tuple(mv(c) for c in blk) for blk in self.blocks]
        self.fc_pi, self.fc_v1, self.fc_v2 = mv(self.fc_pi), mv(self.fc_v1), mv(self.fc_v2)
        return self

    @torch.no_grad()
    def forward(self, boards, valids):
        B = boards.shape[0]
        x = boards.reshape(B, 5, 5, 3).to(self.dtype).permute(0, 3, 1, 2)
        meta = F.relu(torch.addmm(self.meta[1], x[:, 2].reshape(B, 25), self.meta[0]))
        x = F.conv2d(x[:, :2].contiguous(), self.c0[0], self.c0[1], padding=1)
        for (we, be), (wd, bd), (wp, bp) in self.blocks:
            h = F.relu(F.conv2d(x, we, be))
            h = F.relu(F.conv2d(h, wd, bd, padding=1, groups=wd.shape[0]))
            x = F.conv2d(h, wp, bp) + x
        hp = torch.cat([F.relu(F.conv2d(x, self.hp[0], self.hp[1])).flatten(1), meta], dim=1)
        logits = torch.addmm(self.fc_pi[1], hp, self.fc_pi[0]).to(_wide(self.dtype))
        hv = torch.cat([F.relu(F.conv2d(x, self.hv[0], self.hv[1])).flatten(1), meta], dim=1)
        v = torch.tanh(torch.addmm(self.fc_v2[1], F.relu(torch.addmm(self.fc_v1[1], hv, self.fc_v1[0])), self.fc_v2[0]).to(_wide(self.dtype)))
        logits = torch.where(valids.bool(), logits, torch.full_like(logits, -1e8))
        return torch.softmax(logits, dim=1).contiguous(), v.contiguous()



class SantoriniV78Hip(SantoriniV89Hip):
    """SantoriniV78 (with gods: 10 InvertedResidual blocks, A = 1782) evaluated by the engine's kernels (azg_nn_s78_forward,
    csrc/nn_conv5x5.hip.h): one launch for the trunk (MFMA GEMMs for the 1x1 convolutions, in-place depthwise 3x3 on the LDS
    tile) and the value head, one for the 132 x 1782 policy FC (MFMA, 16 samples per workgroup) + masked softmax.  Wraps a SantoriniV78."""

    def __init__(self, base, max_batch=4096, split=True, h2=True, policy2=True):
        """h2 (default): the 1x1 convolutions of the trunk and the depthwise pass on f16 x 2 split-precision operands
        (azg_nn_s78_forward_h2: three MFMAs per product).  Otherwise split: bf16 x 3 (azg_nn_s78_forward_split, 8 samples per
        workgroup, the expanded tile in thirds); False = the f32-MFMA kernel (4 samples per workgroup).
        policy2 (with h2; default): the policy FC as a GEMM launch into the net's own logits workspace + a softmax launch; False = FC +
        softmax in one launch (k_s78_policy_h2, no workspace)"""
        from . import _lib
        self._lib, self.base, self.device, self.split, self.h2 = _lib, base, base.device, bool(split) or bool(h2), bool(h2)
        self.policy2 = self.h2 and bool(policy2)
        self.P, self.A = base.P, base.A
        assert base.dtype == torch.float32 and self.device.type == 'cuda' and len(base.blocks) == 10 and self.A == 1782 and self.P == 2
        ke = _pow2_scale(max(float(we.abs().max()) for (we, _), _, _ in base.blocks))
        kp = _pow2_scale(max(float(wp.abs().max()) for _, _, (wp, _) in base.blocks))
        self.ds_e, self.ds_p = _descale(ke), _descale(kp)

        def thirds(ms, of_k):              # the three 64 x 64 pieces of each [64][192] expand / [192][64] project matrix, each
            # [4 ct][2 chunks of 32][planes][64 lanes][8]: f16 hi / lo of W * 2^k (h2) or bf16 hi / mid / lo
            kind, k = ('h2', kp if of_k else ke) if self.h2 else ('bf16x3', 0)
            return torch.cat([_split_frag(m[64 * t:64 * t + 64] if of_k else m[:, 64 * t:64 * t + 64], kind, k) for m in ms for t in range(3)]).contiguous()
        frag = _frag
        d = self.device
        m0 = torch.zeros((9, 16, 64), dtype=torch.float32, device=d)
        m0[:, :2] = base.c0[0].permute(2, 3, 1, 0).reshape(9, 2, 64)
        assert float(base.c0[1].abs().max()) == 0.0          # the first conv of V78 has no bias and no BatchNorm
        cat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).contiguous()  # noqa: E731
        wfp = torch.zeros((144, 1792), dtype=torch.float32, device=d)      # the policy FC for k_s78_policy: K 132 -> 144, N 1782 -> 1792
        wfp[:132, :1782] = base.fc_pi[0]
        bfp = torch.zeros(1792, dtype=torch.float32, device=d)
        bfp[:1782] = base.fc_pi[1]
        if self.h2:                        # the policy FC on f16 x 2 operands too (k_s78_policy_h2): K 132 -> 160, hi / lo fragments + the descale
            kf = _pow2_scale(base.fc_pi[0].abs().max())
            fr = _split_frag(_pad(base.fc_pi[0], (160, 1792)), 'h2', kf).view(torch.uint8)
            tail = torch.tensor([_descale(kf), 0.0, 0.0, 0.0], dtype=torch.float32, device=d).view(torch.uint8)
            wfp_h2 = torch.cat([fr, tail]).contiguous()
        keep = [frag(m0.reshape(144, 64).contiguous()),
                (thirds([we.reshape(192, 64).t() for (we, _), _, _ in base.blocks], False) if self.split else
                 cat([frag(we.reshape(192, 64).t().contiguous()) for (we, _), _, _ in base.blocks])), cat([be for (_, be), _, _ in base.blocks]),
                cat([wd.reshape(192, 9) for _, (wd, _), _ in base.blocks]), cat([bd for _, (_, bd), _ in base.blocks]),
                (thirds([wp.reshape(64, 192).t() for _, _, (wp, _) in base.blocks], True) if self.split else
                 cat([frag(wp.reshape(64, 192).t().contiguous()) for _, _, (wp, _) in base.blocks])), cat([bp for _, _, (_, bp) in base.blocks]),
                base.meta[0].contiguous(), base.meta[1].contiguous(),
                base.hp[0].reshape(4, 64).t().contiguous(), base.hp[1].contiguous(), (wfp_h2 if self.h2 else frag(wfp)), bfp,
                base.hv[0].reshape(2, 64).t().contiguous(), base.hv[1].contiguous(), base.fc_v1[0].contiguous(), base.fc_v1[1].contiguous(),
                base.fc_v2[0].contiguous(), base.fc_v2[1].contiguous()]
        assert len(keep) == 19 and tuple(base.fc_pi[0].shape) == (132, 1782) and tuple(base.fc_v1[0].shape) == (82, 64)
        self._keep = keep
        self.ptrs = (C.c_void_p * 19)(*[t.data_ptr() for t in keep])
        self._alloc(max_batch)

    def _alloc(self, B):
        super()._alloc(B)
        if self.policy2:               # the raw logits between the policy GEMM and the softmax: an activation buffer like pi and v
            self.logits = torch.empty((B, 1792), dtype=torch.float32, device=self.device)

    def _launch(self, boards, valids, B, stream):
        L = self._lib.lib()
        if self.h2:
            self._lib.check(L.azg_nn_s78_forward_h2(boards, valids, self.ptrs, self.ds_e, self.ds_p, 10, self.A, self.P, B, _ptr(self.pi),
                                                    _ptr(self.v), _ptr(self.logits) if self.policy2 else None, stream))
            return
        fwd = L.azg_nn_s78_forward_split if self.split else L.azg_nn_s78_forward
        self._lib.check(fwd(boards, valids, self.ptrs, 10, self.A, self.P, B, _ptr(self.pi), _ptr(self.v), stream))


class AbaloneV21(_TorchNet):
    """abalone/AbaloneNNet.py nn_version 21 (:120-160, forward :173-201) -- the net of pretrained_BelgianDaisy.pt: the 3 spatial
    planes (marbles of each player, hex mask) of the (9, 9, 4) board -> conv3x3(3->24)+BN+ReLU -> 4 torchvision InvertedResidual
    blocks (1x1 expand 24->48 + BN + ReLU, depthwise 3x3 + BN + ReLU, 1x1 project + BN, residual; no SE) -> policy 1x1 conv
    24->42 + BN laid out [9][9][42]; value 1x1 conv 24->4 + BN + ReLU flattened channel-major, concatenated with a 16-wide
    embedding of the 6 metadata values (Linear(6,16)+ReLU), -> 64 -> P.  BatchNorm (eps 1e-5) folded; plain torch ops."""

    def __init__(self, state_dict, num_players=2, device='cuda:0', dtype=torch.float32):
        sd = {k: torch.as_tensor(v).to(_wide(dtype)) for k, v in state_dict.items()}
        self.P, self.A = num_players, 81 * sd['head_PI.0.weight'].shape[0]

        def conv_bn(conv, bn):
            s, b = _fold_bn(sd, bn)
            return (sd[conv + '.weight'] * s[:, None, None, None]).contiguous(), b
        self.c0 = conv_bn('first_layer.0', 'first_layer.1')
        self.blocks = []
        i = 0
        while 'trunk.%d.block.0.0.weight' % i in sd:
            self.blocks.append(tuple(conv_bn('trunk.%d.block.%d.0' % (i, j), 'trunk.%d.block.%d.1' % (i, j)) for j in range(3)))
            i += 1
        self.hp = conv_bn('head_PI.0', 'head_PI.1')
        self.hv = conv_bn('head_V_conv.0', 'head_V_conv.1')
        self.meta = (sd['meta_fc.0.weight'].t().contiguous(), sd['meta_fc.0.bias'])
        self.fc_v1 = (sd['head_V_fc.0.weight'].t().contiguous(), sd['head_V_fc.0.bias'])
        self.fc_v2 = (sd['head_V_fc.2.weight'].t().contiguous(), sd['head_V_fc.2.bias'])
        self.to(device, dtype)

    def to(self, device, dtype=torch.float32):
        self.device, self.dtype = torch.device(device), dtype
        mv = lambda pr: tuple(t.to(self.device, dtype) for t in pr)  # noqa: E731
        self.c0, self.hp, self.hv, self.meta = mv(self.c0), mv(self.hp), mv(self.hv), mv(self.meta)
        self.blocks = [tuple(mv(c) for c in blk) for blk in self.blocks]
        self.fc_v1, self.fc_v2 = mv(self.fc_v1), mv(self.fc_v2)
        return self

    @torch.no_grad()
    def forward(self, boards, valids):
        B = boards.shape[0]
        x = boards.reshape(B, 9, 9, 4).to(self.dtype)
        meta = F.relu(torch.addmm(self.meta[1], x[:, 0, 0:6, 3], self.meta[0]))
        x = F.relu(F.conv2d(x[..., :3].permute(0, 3, 1, 2).contiguous(), self.c0[0], self.c0[1], padding=1))
        for (we, be), (wd, bd), (wp, bp) in self.blocks:
            h = F.relu(F.conv2d(x, we, be))
            h = F.relu(F.conv2d(h, wd, bd, padding=1, groups=wd.shape[0]))
            x = F.conv2d(h, wp, bp) + x
        logits = F.conv2d(x, self.hp[0], self.hp[1]).permute(0, 2, 3, 1).reshape(B, self.A).to(_wide(self.dtype))
        hv = torch.cat([F.relu(F.conv2d(x, self.hv[0], self.hv[1])).flatten(1), meta], dim=1)
        v = torch.tanh(torch.addmm(self.fc_v2[1], F.relu(torch.addmm(self.fc_v1[1], hv, self.fc_v1[0])), self.fc_v2[0]).to(_wide(self.dtype)))
        logits = torch.where(valids.bool(), logits, torch.full_like(logits, -1e8))
        return torch.softmax(logits, dim=1).contiguous(), v.contiguous()


class AbaloneV21Hip(_EngineNet):
    """AbaloneV21 (4 InvertedResidual blocks on the 9 x 9 grid, A = 3402) evaluated by the engine's one-launch kernel
    (azg_nn_aba21_forward, csrc/nn_abalone.hip.h: f32 MFMA GEMMs for the convolutions, the depthwise 3x3 on the vector ALUs, heads
    and masked softmax in the same launch) instead of ~20 MIOpen / hipBLASLt launches.  Wraps an AbaloneV21; static pi / v buffers
    (HIP-graph capture of the engine's rounds)."""
    _FN, S = 'azg_nn_aba21_forward', 324

    def __init__(self, base, max_batch=4096):
        from . import _lib
        self._lib, self.base, self.device = _lib, base, base.device
        self.P, self.A = base.P, base.A
        assert base.dtype == torch.float32 and self.device.type == 'cuda' and len(base.blocks) == 4 and self.A == 3402 and self.P == 2
        keep = self.pack(base)
        self._keep = keep
        self.ptrs = (C.c_void_p * 16)(*[t.data_ptr() for t in keep])
        self._alloc(max_batch)

    @staticmethod
    def pack(base):
        """the 16 weight tensors of azg_nn_aba21_forward (include/azg.h), on base's device"""
        d = base.device

        def frag(m, G, nct):               # [K][N] -> [nct][G][64 lanes], element = m[G * (lane >> 4) + j][16 * ct + (lane & 15)] (zero padded)
            z = torch.zeros((4 * G, 16 * nct), dtype=torch.float32, device=d)
            z[:m.shape[0], :m.shape[1]] = m
            return z.view(4, G, nct, 16).permute(2, 1, 0, 3).contiguous().view(-1)
        cat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).contiguous()  # noqa: E731
        wh = torch.cat([base.hp[0].reshape(42, 24).t(), base.hv[0].reshape(4, 24).t()], dim=1)
        bh = torch.zeros(48, dtype=torch.float32, device=d)
        bh[:42], bh[42:46] = base.hp[1], base.hv[1]
        keep = [frag(base.c0[0].permute(2, 3, 1, 0).reshape(27, 24), 8, 2), base.c0[1].contiguous(),
                cat([frag(we.reshape(48, 24).t(), 6, 3) for (we, _), _, _ in base.blocks]), cat([be for (_, be), _, _ in base.blocks]),
                cat([wd.reshape(48, 9) for _, (wd, _), _ in base.blocks]), cat([bd for _, (_, bd), _ in base.blocks]),
                cat([frag(wp.reshape(24, 48).t(), 12, 2) for _, _, (wp, _) in base.blocks]), cat([bp for _, _, (_, bp) in base.blocks]),
                frag(wh, 6, 3), bh, base.meta[0].contiguous(), base.meta[1].contiguous(),
                base.fc_v1[0].contiguous(), base.fc_v1[1].contiguous(), base.fc_v2[0].contiguous(), base.fc_v2[1].contiguous()]
        assert tuple(base.fc_v1[0].shape) == (340, 64) and tuple(base.meta[0].shape) == (6, 16)
        return keep

    def _ints(self):
        return (4, self.A, self.P)


class SmallworldV62(_TorchNet):
    """smallworld/SmallworldNNet.py nn_version 62 (:246-254, stem :86-137, heads :139-180, forward :268-294) -- the net of all three shipped
    checkpoints (pretrained_{2,3,4}pl.pt): InputStem over the (N, 8) tokens -> 48, three post-norm TransformerEncoderLayers (3 heads of 16,
    feed-forward 192, ReLU, LayerNorm eps 1e-5, no mask), ActionSlicerHead (local 48 -> 5 on the nA area tokens, mean of the other tokens
    -> global 48 -> 16 and value 48 -> P), masked softmax, tanh.  The stem's out_proj is linear over the concatenation of its five parts,
    so it is folded (in f64) into three lookup tables and one 21 -> 48 projection; the 1/4 attention scale is folded into the Q rows of
    in_proj (exact).  Plain torch ops."""
    N_TOKENS = {2: 40, 3: 52, 4: 66}
    _TENSORS = ('t_ppl', 't_pwr', 't_pl', 'w_st', 'b_st', 'ln_s', 'local', 'glob', 'value')

    def __init__(self, state_dict, num_players=2, device='cuda:0', dtype=torch.float32):
        sd = {k: torch.as_tensor(v).double() for k, v in state_dict.items() if not k.endswith('powers_of_2')}
        self.P, self.N = num_players, self.N_TOKENS[num_players]
        self.nA = {2: 23, 3: 30, 4: 39}[num_players]
        self.A = 5 * self.nA + 16
        assert sd['head.value_head.weight'].shape[0] == num_players
        wo, bo = sd['stem.out_proj.weight'], sd['stem.out_proj.bias']            # [48][240]: ppl | pwr | player | num | bits
        sl = [wo[:, 48 * k:48 * (k + 1)] for k in range(5)]
        self.t_ppl = sd['stem.emb_ppl.weight'] @ sl[0].t()
        self.t_pwr = sd['stem.emb_pwr.weight'] @ sl[1].t()
        self.t_pl = sd['stem.emb_player.weight'] @ sl[2].t()
        self.w_st = torch.cat([(sl[3] @ sd['stem.num_proj.weight']).t(), (sl[4] @ sd['stem.bit_proj.weight']).t()])     # [21][48]
        self.b_st = bo + sl[3] @ sd['stem.num_proj.bias'] + sl[4] @ sd['stem.bit_proj.bias']
        self.ln_s = (sd['stem.norm.weight'], sd['stem.norm.bias'])
        self.layers = []
        i = 0
        while 'trunk.layers.%d.linear1.weight' % i in sd:
            q = lambda n: sd['trunk.layers.%d.%s' % (i, n)]  # noqa: E731
            scale = torch.ones(144, dtype=torch.float64)
            scale[:48] = 0.25                                                           # 1 / sqrt(16): a power of two, exact
            self.layers.append(dict(w_in=q('self_attn.in_proj_weight') * scale[:, None], b_in=q('self_attn.in_proj_bias') * scale,
                                    w_o=q('self_attn.out_proj.weight'), b_o=q('self_attn.out_proj.bias'),
                                    ln1=(q('norm1.weight'), q('norm1.bias')), w1=q('linear1.weight'), b1=q('linear1.bias'),
                                    w2=q('linear2.weight'), b2=q('linear2.bias'), ln2=(q('norm2.weight'), q('norm2.bias'))))
            i += 1
        self.local = (sd['head.local_head.weight'], sd['head.local_head.bias'])
        self.glob = (sd['head.global_head.weight'], sd['head.global_head.bias'])
        self.value = (sd['head.value_head.weight'], sd['head.value_head.bias'])
        self.to(device, dtype)

    def to(self, device, dtype=torch.float32):
        self.device, self.dtype = torch.device(device), dtype
        mv = lambda t: tuple(mv(x) for x in t) if isinstance(t, tuple) else t.to(self.device, dtype).contiguous()  # noqa: E731
        for n in self._TENSORS:
            setattr(self, n, mv(getattr(self, n)))
        self.layers = [{k: mv(t) for k, t in lay.items()} for lay in self.layers]
        self.shifts = torch.arange(8, device=self.device)
        return self

    @torch.no_grad()
    def forward(self, boards, valids):
        B = boards.shape[0]
        b = boards.reshape(B, self.N, 8)
        c = b.to(torch.int64)
        e1, e2, e7 = (c[..., 1] + 15).clamp(0, 30), (c[..., 2] + 20).clamp(0, 40), (c[..., 7] + 1).clamp(0, 5)
        num = torch.cat([b[..., 0:1], b[..., 3:7]], dim=-1).to(torch.float32) / 10.0       # (slices, not a list index: no host copy in graph capture)
        bits = torch.cat([(c[..., 3:4] >> self.shifts) & 1, (c[..., 4:5] >> self.shifts) & 1], dim=-1)   # bits of the two's-complement pattern
        f = torch.cat([num.to(self.dtype), bits.to(self.dtype)], dim=-1)
        x = self.t_ppl[e1] + self.t_pwr[e2] + self.t_pl[e7] + f @ self.w_st + self.b_st
        x = F.layer_norm(x, (48,), *self.ln_s, eps=1e-5)
        for lay in self.layers:
            qkv = F.linear(x, lay['w_in'], lay['b_in']).view(B, self.N, 3, 3, 16)                       # (token, q|k|v, head, dim)
            q, k, v = (qkv[:, :, j].transpose(1, 2) for j in range(3))                                   # [B][head][N][16]
            o = torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v
            o = F.linear(o.transpose(1, 2).reshape(B, self.N, 48), lay['w_o'], lay['b_o'])
            x = F.layer_norm(x + o, (48,), *lay['ln1'], eps=1e-5)
            y = F.linear(F.relu(F.linear(x, lay['w1'], lay['b1'])), lay['w2'], lay['b2'])
            x = F.layer_norm(x + y, (48,), *lay['ln2'], eps=1e-5)
        nA = self.nA
        loc = F.linear(x[:, :nA], *self.local)                                                           # [B][nA][5]
        g = x[:, nA:].mean(dim=1)
        gl = F.linear(g, *self.glob)
        logits = torch.cat([loc[..., 0], loc[..., 1], loc[..., 2], loc[..., 3], gl[:, 0:8], loc[..., 4], gl[:, 8:16]], dim=1).to(_wide(self.dtype))
        v = torch.tanh(F.linear(g, *self.value).to(_wide(self.dtype)))
        logits = torch.where(valids.bool(), logits, torch.full_like(logits, -1e8))
        return torch.softmax(logits, dim=1).contiguous(), v.contiguous()


class SmallworldV62Hip(_EngineNet):
    """SmallworldV62 (3 transformer layers, P = 2 / 3 / 4) evaluated by the engine's one-launch kernel (azg_nn_sw62_forward,
    csrc/nn_smallworld.hip.h: f32 MFMA for the per-token GEMMs and the two attention products, stem / softmax / LayerNorm / heads on
    the vector ALUs, masked softmax in the same launch) instead of ~40 torch launches.  Wraps a SmallworldV62; static pi / v buffers
    (HIP-graph capture of the engine's rounds)."""
    _FN = 'azg_nn_sw62_forward'

    def __init__(self, base, max_batch=4096):
        from . import _lib
        self._lib, self.base, self.device = _lib, base, base.device
        self.P, self.A, self.N, self.S = base.P, base.A, base.N, 8 * base.N
        assert base.dtype == torch.float32 and self.device.type == 'cuda' and len(base.layers) == 3
        keep = self.pack(base)
        self._keep = keep
        self.ptrs = (C.c_void_p * 25)(*[t.data_ptr() for t in keep])
        self._alloc(max_batch)

    @staticmethod
    def frag(wt, nct):
        """W^T [K][Nout] (K a multiple of 16) -> [nct][K / 4][64 lanes], element [ct][m][lane] = W^T[16 (m >> 2) + 4 (lane >> 4) + (m & 3)]
        [16 ct + (lane & 15)] (zero padded): the k order of every GEMM of nn_smallworld.hip.h"""
        K = wt.shape[0]
        z = torch.zeros((K, 16 * nct), dtype=torch.float32, device=wt.device)
        z[:, :wt.shape[1]] = wt
        return z.view(K // 16, 4, 4, nct, 16).permute(3, 0, 2, 1, 4).contiguous().view(-1)

    @staticmethod
    def pack(base):
        """the 25 weight tensors of azg_nn_sw62_forward (include/azg.h), on base's device"""
        fr, L = SmallworldV62Hip.frag, base.layers
        cat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).contiguous()  # noqa: E731
        keep = [base.t_ppl, base.t_pwr, base.t_pl, base.w_st, base.b_st, base.ln_s[0], base.ln_s[1],
                cat([fr(y['w_in'].t(), 9) for y in L]), cat([y['b_in'] for y in L]),
                cat([fr(y['w_o'].t(), 3) for y in L]), cat([y['b_o'] for y in L]),
                cat([y['ln1'][0] for y in L]), cat([y['ln1'][1] for y in L]),
                cat([fr(y['w1'].t(), 12) for y in L]), cat([y['b1'] for y in L]),
                cat([fr(y['w2'].t(), 3) for y in L]), cat([y['b2'] for y in L]),
                cat([y['ln2'][0] for y in L]), cat([y['ln2'][1] for y in L]),
                base.local[0].t().contiguous(), base.local[1], base.glob[0].t().contiguous(), base.glob[1],
                base.value[0].t().contiguous(), base.value[1]]
        assert tuple(base.w_st.shape) == (21, 48) and tuple(base.t_ppl.shape) == (31, 48) and tuple(L[0]['w1'].shape) == (192, 48)
        return [t.to(torch.float32).contiguous() for t in keep]

    def _ints(self):
        return (3, self.A, self.P)


class AkropolisV31(_TorchNet):
    """akropolis/AkropolisNNet.py nn_version 31 (constructor :91-146, input slicing :377-388, forward :573-622) -- the net of all three
    shipped checkpoints (pretrained_{2,3,4}pl.pt).  Per player, the board [embed(descr) (3), height, tileID] -> conv3x3(5->8) + BN +
    Hardswish -> conv3x3(8->8) + BN + Hardswish on 13 x 13 (shared weights); s1 = Linear(15P->16)(scores), g1 = Hardswish(BN(Linear(2->8)
    (globals))); proj_p = a kernel-1 InvertedResidual (8P + 24 -> 32, depthwise scale, SE 32->8->32, -> 16, no residual) over the cells;
    per construction-site tile c: t = Hardswish(Conv1d(3->32, k 3)(embed(codes))), f3 = [t, s1, g1], a = Hardswish(BN(proj_i(f3))),
    h = proj_o(f3) as [6][16]; logit[c, cell, o] = sum_r a[c,r] p[cell,r] h[c,o,r] (action c*1014 + cell*6 + o); masked softmax; value
    head on flatten(f3).  Every BatchNorm (eps 1e-5) folded; the s1 / g1 channels of proj_p's first 1x1 are constant over the cells and
    folded into one per-sample 32-vector; the policy is one (169 x 16) x (16 x 6 CS) product per sample with W_c[o][r] = a[c,r] h[c,o,r]
    (einsum: the reference's (N, CS, 6, 13, 13, 16) product is never formed).  Plain torch ops."""
    _TENSORS = ('embed', 'w1', 'b1', 'w2', 'b2', 'ws', 'bs', 'wg', 'bg', 'wc', 'bc', 'we', 'wec', 'be', 'dws', 'dwb', 'fc1', 'fc1b', 'fc2',
                'fc2b', 'wp', 'bp', 'wi', 'bi', 'wo', 'bo', 'wv1', 'bv1', 'wv2', 'bv2', 'wv3', 'bv3')

    def __init__(self, state_dict, num_players=2, device='cuda:0', dtype=torch.float32):
        sd = {k: torch.as_tensor(v).double() for k, v in state_dict.items() if not k.endswith('num_batches_tracked')}
        P = self.P = num_players
        self.C, self.CS = 3 * P + 2, P + 2
        self.S, self.A = 169 * self.C, 1014 * self.CS
        assert sd['final_layers_V.6.weight'].shape[0] == P and sd['dense_scores.0.weight'].shape[1] == 15 * P

        def conv_bn(conv, bn, bias=True):
            s, b = _fold_bn(sd, bn)
            w = sd[conv + '.weight']
            return w * s.view((-1,) + (1,) * (w.dim() - 1)), (sd[conv + '.bias'] * s if bias else 0) + b
        self.embed = sd['embed.weight']                                                     # [12][3]
        self.w1, self.b1 = conv_bn('conv2d_boards.0', 'conv2d_boards.1')                    # [8][5][3][3]
        self.w2, self.b2 = conv_bn('conv2d_boards.3', 'conv2d_boards.4')                    # [8][8][3][3]
        self.ws, self.bs = sd['dense_scores.0.weight'].t(), sd['dense_scores.0.bias']       # [15P][16]
        wg, self.bg = conv_bn('dense_globs.0', 'dense_globs.1')
        self.wg = wg.t()                                                                    # [2][8]
        self.wc, self.bc = sd['conv1d_constr.0.weight'], sd['conv1d_constr.0.bias']        # [32][3][3] (out, emb, position)
        w0, b0 = conv_bn('proj_p.0.block.0.0', 'proj_p.0.block.0.1', bias=False)
        w0 = w0.reshape(32, 8 * P + 24)
        self.we, self.wec, self.be = w0[:, :8 * P].t(), w0[:, 8 * P:].t(), b0              # [8P][32], [24][32] (s1 | g1), [32]
        dw, self.dwb = conv_bn('proj_p.0.block.1.0', 'proj_p.0.block.1.1', bias=False)
        self.dws = dw.reshape(32)                                                           # the depthwise 1x1: a per-channel scale
        self.fc1, self.fc1b = sd['proj_p.0.block.2.fc1.weight'].reshape(8, 32).t(), sd['proj_p.0.block.2.fc1.bias']
        self.fc2, self.fc2b = sd['proj_p.0.block.2.fc2.weight'].reshape(32, 8).t(), sd['proj_p.0.block.2.fc2.bias']
        wp, self.bp = conv_bn('proj_p.0.block.3.0', 'proj_p.0.block.3.1', bias=False)
        self.wp = wp.reshape(16, 32).t()                                                    # [32][16]
        wi, self.bi = conv_bn('proj_i', 'b1n.0')                                            # b1n folded into proj_i
        self.wi = wi.t()                                                                    # [56][16]
        self.wo, self.bo = sd['proj_o.weight'].t(), sd['proj_o.bias']                      # [56][96]: h[o][r] = column 16 o + r
        wv1, self.bv1 = conv_bn('final_layers_V.1', 'final_layers_V.2')
        self.wv1 = wv1.t()                                                                  # [CS * 56][16]
        self.wv2, self.bv2 = sd['final_layers_V.4.weight'].t(), sd['final_layers_V.4.bias']
        self.wv3, self.bv3 = sd['final_layers_V.6.weight'].t(), sd['final_layers_V.6.bias']
        self.to(device, dtype)

    def to(self, device, dtype=torch.float32):
        self.device, self.dtype = torch.device(device), dtype
        for n in self._TENSORS:
            setattr(self, n, getattr(self, n).to(self.device, dtype).contiguous())
        return self

    def context(self, x):
        """x [B][13][13][C] (self.dtype) -> s1 [B][16], g1 [B][8], f3 [B][CS][56]"""
        P, CS = self.P, self.CS
        B = x.shape[0]
        s1 = x[:, 0:3 * P, 0:5, 3 * P].reshape(B, 15 * P) @ self.ws + self.bs
        g1 = F.hardswish(x[:, CS + 1, 0:2, 3 * P + 1] @ self.wg + self.bg)
        ce = self.embed[x[:, 0:CS, 0:3, 3 * P + 1].clamp(0, 11).long()]                   # [B][CS][3 positions][3]
        t = F.hardswish(torch.einsum('bcke,oek->bco', ce, self.wc) + self.bc)
        f3 = torch.cat([t, s1[:, None].expand(B, CS, 16), g1[:, None].expand(B, CS, 8)], dim=2)
        return s1, g1, f3

    @torch.no_grad()
    def forward(self, boards, valids):
        P, CS = self.P, self.CS
        B = boards.shape[0]
        x = boards.reshape(B, 13, 13, self.C).to(self.dtype)
        s1, g1, f3 = self.context(x)
        # the P boards, shared convolutions: [B * P][5][13][13]
        e = self.embed[x[..., 0:P].clamp(0, 11).long()]                                     # [B][13][13][P][3]
        xb = torch.cat([e, x[..., P:2 * P, None], x[..., 2 * P:3 * P, None]], dim=4)       # [B][13][13][P][5]
        xb = xb.permute(0, 3, 4, 1, 2).reshape(B * P, 5, 13, 13)
        hb = F.hardswish(F.conv2d(xb, self.w1, self.b1, padding=1))
        hb = F.hardswish(F.conv2d(hb, self.w2, self.b2, padding=1))                        # [B * P][8][13][13]
        fb = hb.reshape(B, P * 8, 169).transpose(1, 2)                                      # [B][169][8P], channel 8 i + k of player i
        c0 = torch.cat([s1, g1], dim=1) @ self.wec + self.be                               # proj_p's s1 / g1 channels: one 32-vector per sample
        d = F.hardswish(F.hardswish(fb @ self.we + c0[:, None]) * self.dws + self.dwb)      # [B][169][32]
        sc = F.hardsigmoid(F.relu(d.mean(dim=1) @ self.fc1 + self.fc1b) @ self.fc2 + self.fc2b)
        p = (d * sc[:, None]) @ self.wp + self.bp                                           # [B][169][16]
        a = F.hardswish(f3 @ self.wi + self.bi)                                             # [B][CS][16]
        wc = a[:, :, None, :] * (f3 @ self.wo + self.bo).view(B, CS, 6, 16)               # W_c [B][CS][6][16]
        logits = torch.einsum('bnr,bcor->bcno', p, wc).reshape(B, self.A).to(_wide(self.dtype))
        v = F.hardswish(f3.reshape(B, CS * 56) @ self.wv1 + self.bv1)
        v = torch.tanh((F.hardswish(v @ self.wv2 + self.bv2) @ self.wv3 + self.bv3).to(_wide(self.dtype)))
        logits = torch.where(valids.bool(), logits, torch.full_like(logits, -1e8))
        return torch.softmax(logits, dim=1).contiguous(), v.contiguous()


class AkropolisV31Hip(_EngineNet):
    """AkropolisV31 (P = 2 / 3 / 4) evaluated by the engine's one-launch kernel (azg_nn_akr31_forward, csrc/nn_akropolis.hip.h: one
    workgroup per sample, one cell per lane, the whole forward and the masked softmax on the vector ALUs) instead of ~50 torch
    launches.  Wraps an AkropolisV31; static pi / v buffers (HIP-graph capture of the engine's rounds)."""
    _FN = 'azg_nn_akr31_forward'

    @staticmethod
    def layout(P):
        """the three packed weight blocks of azg_nn_akr31_forward (include/azg.h, Akr31<P> offsets in nn_akropolis.hip.h): per block
        the (name, shape) of its tensors in order"""
        CS = P + 2
        return ([('ws', (15 * P, 16)), ('bs', (16,)), ('wg', (2, 8)), ('bg', (8,)), ('tc', (3, 12, 32)), ('bc', (32,)), ('wi', (56, 16)),
                 ('bi', (16,)), ('wo', (56, 96)), ('bo', (96,)), ('wec', (24, 32)), ('be', (32,)), ('wv1', (56 * CS, 16)), ('bv1', (16,)),
                 ('wv2', (16, 16)), ('bv2', (16,)), ('wv3', (16, P)), ('bv3', (P,))],
                [('t1', (9, 12, 8)), ('w1x', (9, 2, 8)), ('b1', (8,)), ('w2', (9, 8, 8)), ('b2', (8,)), ('we', (8 * P, 32))],
                [('dws', (32,)), ('dwb', (32,)), ('fc1', (32, 8)), ('fc1b', (8,)), ('fc2', (8, 32)), ('fc2b', (32,)), ('wp', (32, 16)),
                 ('bp', (16,))])

    @staticmethod
    def folded(base):
        """name -> tensor of every operand the kernel reads, in base's dtype: base's folds plus the embedding folded into the per-tap
        code tables of conv1 (t1) and the per-position code tables of conv1d_constr (tc)"""
        w1 = base.w1.permute(2, 3, 1, 0).reshape(9, 5, 8)                                  # [tap = 3 ky + kx][in][out]
        f = {n: getattr(base, n) for n in ('ws', 'bs', 'wg', 'bg', 'bc', 'wi', 'bi', 'wo', 'bo', 'wec', 'be', 'wv1', 'bv1', 'wv2', 'bv2',
                                           'wv3', 'bv3', 'b1', 'b2', 'we', 'dws', 'dwb', 'fc1', 'fc1b', 'fc2', 'fc2b', 'wp', 'bp')}
        f['t1'] = torch.einsum('ce,teo->tco', base.embed, w1[:, 0:3])                       # [9][12][8]: embed(code) through tap t
        f['w1x'] = w1[:, 3:5]                                                                # [9][2][8]: height, tileID
        f['w2'] = base.w2.permute(2, 3, 1, 0).reshape(9, 8, 8)                              # [tap][in][out]
        f['tc'] = torch.einsum('ce,oek->kco', base.embed, base.wc)                          # [3][12][32]: embed(code) at position k
        return f

    @staticmethod
    def pack(base):
        """the three f32 weight blocks of azg_nn_akr31_forward, on base's device"""
        f = AkropolisV31Hip.folded(base)
        blocks = []
        for blk in AkropolisV31Hip.layout(base.P):
            for n, shape in blk:
                assert tuple(f[n].shape) == shape, (n, tuple(f[n].shape), shape)
            blocks.append(torch.cat([f[n].reshape(-1) for n, _ in blk]).to(torch.float32).contiguous())
        return blocks

    @staticmethod
    def unpack(blocks, P):
        """inverse of pack: name -> tensor view"""
        out = {}
        for blk, t in zip(AkropolisV31Hip.layout(P), blocks):
            o = 0
            for n, shape in blk:
                k = int(np.prod(shape))
                out[n] = t[o:o + k].view(shape)
                o += k
            assert o == t.numel()
        return out

    def __init__(self, base, max_batch=4096):
        from . import _lib
        self._lib, self.base, self.device = _lib, base, base.device
        self.P, self.A, self.S = base.P, base.A, base.S
        assert base.dtype == torch.float32 and self.device.type == 'cuda'
        keep = self.pack(base)
        self._keep = keep
        self.ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in keep])
        self._alloc(max_batch)

    def _ints(self):
        return (self.P, self.A)


class BotanikV1x(_TorchNet):
    """botanik/BotanikNNet.py nn_version 10 (:105-160) and 11 (:162-237), forward :251-292: the (66, 5, 7) board, rows 0..25 read.
    1-d branch: rows 0..5 as (C = 7, L = 30) -> first_layer_1d (Linear 7 -> 7 + BN) -> trunk_1d InvertedResidual1d(7, 21, 7, 30, ReLU, SE
    avg: the reference passes "RE" as use_se, which is truthy) -> per head InvertedResidual1d(7, 21, 7, 30, Hardswish, SE max) + Flatten +
    Linear(210, 428 | 2).  Machine branch (mach0; V11 also mach1, separate weights): the first 343 bytes of rows 6..15 (16..25) as
    (H, W, C) = (7, 7, 7) -> conv3x3 7 -> 16 -> one torchvision InvertedResidual 16 -> 32 -> 16 (ReLU, no SE) -> per head three
    InvertedResidual 16 -> 48 -> 16 (Hardswish, SE) + Flatten + Linear(784, 428 | 2).  The branch outputs are summed, then
    final_layers_PI (428 -> 428 + ReLU -> 428), masked softmax; final_layers_V (2 -> 2 + ReLU -> 2), tanh.  The version is 11 when the
    state_dict has first_layer_mach1.weight.  BatchNorm (eps 1e-5) folded; plain torch ops."""
    A, P = 428, 2

    def __init__(self, state_dict, device='cuda:0', dtype=torch.float32):
        sd = {k: torch.as_tensor(v).to(_wide(dtype)) for k, v in state_dict.items()}
        self.n_mach = 2 if 'first_layer_mach1.weight' in sd else 1
        self.version = 9 + self.n_mach
        t = {}

        def lin_bn(pre):                 # LinearNormActivation: Linear (no bias) + BatchNorm1d over its outputs
            s, b = _fold_bn(sd, pre + '.norm')
            return sd[pre + '.linear.weight'] * s[:, None], b
        t['1d.W0'], t['1d.b0'] = lin_bn('first_layer_1d')
        for j, pre in enumerate(('trunk_1d.0', 'output_layers_PI_1d.0', 'output_layers_V_1d.0')):
            k = '1d.%d.' % j
            t[k + 'We'], t[k + 'be'] = lin_bn(pre + '.expand')
            t[k + 'sd'], t[k + 'bd'] = _fold_bn(sd, pre + '.depthwise.norm')
            t[k + 'Wt'] = sd[pre + '.depthwise.linear.weight']
            for n in ('1', '2'):
                t[k + 'W' + n], t[k + 'b' + n] = sd[pre + '.se.fc%s.weight' % n], sd[pre + '.se.fc%s.bias' % n]
            t[k + 'Wp'], t[k + 'bp'] = lin_bn(pre + '.project')
        for h, pre in (('pi', 'output_layers_PI'), ('v', 'output_layers_V')):
            t[h + '1d.W'], t[h + '1d.b'] = sd[pre + '_1d.2.weight'], sd[pre + '_1d.2.bias']

        def conv_bn(pre):
            s, b = _fold_bn(sd, pre + '.1')
            return sd[pre + '.0.weight'] * s[:, None, None, None], b
        for m in range(self.n_mach):
            k = 'm%d.' % m
            t[k + 'c0'] = sd['first_layer_mach%d.weight' % m]
            for j, n in enumerate(('e', 'd', 'p')):
                t[k + 't.w' + n], t[k + 't.b' + n] = conv_bn('trunk_mach%d.0.block.%d' % (m, j))
            for h, pre in enumerate(('output_layers_PI_mach%d' % m, 'output_layers_V_mach%d' % m)):
                for b in range(3):
                    q, blk = k + 'h%d.' % (3 * h + b), '%s.%d.block.' % (pre, b)
                    t[q + 'we'], t[q + 'be'] = conv_bn(blk + '0')
                    t[q + 'wd'], t[q + 'bd'] = conv_bn(blk + '1')
                    for n in ('1', '2'):
                        t[q + 'w' + n], t[q + 'b' + n] = sd[blk + '2.fc%s.weight' % n], sd[blk + '2.fc%s.bias' % n]
                    t[q + 'wp'], t[q + 'bp'] = conv_bn(blk + '3')
                t[('pi' if h == 0 else 'v') + k + 'W'], t[('pi' if h == 0 else 'v') + k + 'b'] = sd[pre + '.4.weight'], sd[pre + '.4.bias']
        for n, pre in (('f1', 'final_layers_PI.0'), ('f2', 'final_layers_PI.2'), ('fv1', 'final_layers_V.0'), ('fv2', 'final_layers_V.2')):
            t[n + '.W'], t[n + '.b'] = sd[pre + '.weight'], sd[pre + '.bias']
        self.t = {k: v.contiguous() for k, v in t.items()}
        self.to(device, dtype)

    def to(self, device, dtype=torch.float32):
        self.device, self.dtype = torch.device(device), dtype
        self.t = {k: v.to(self.device, dtype) for k, v in self.t.items()}
        return self

    def _block1d(self, k, x, hs, maxpool):              # x [B, 7, 30]
        t, act = self.t, (F.hardswish if hs else F.relu)
        h = act(torch.einsum('ec,bcl->bel', t[k + 'We'], x) + t[k + 'be'][:, None])
        h = act(torch.matmul(h, t[k + 'Wt'].t()) * t[k + 'sd'][:, None] + t[k + 'bd'][:, None])
        p = h.amax(dim=2) if maxpool else h.mean(dim=2)
        s = F.hardsigmoid(F.linear(F.relu(F.linear(p, t[k + 'W1'], t[k + 'b1'])), t[k + 'W2'], t[k + 'b2']))
        return torch.einsum('ce,bel->bcl', t[k + 'Wp'], h * s[:, :, None]) + t[k + 'bp'][:, None] + x

    def _block2d(self, q, x):                          # torchvision InvertedResidual 16 -> 48 -> 16, Hardswish, SE
        t = self.t
        h = F.hardswish(F.conv2d(x, t[q + 'we'], t[q + 'be']))
        h = F.hardswish(F.conv2d(h, t[q + 'wd'], t[q + 'bd'], padding=1, groups=h.shape[1]))
        s = F.hardsigmoid(F.conv2d(F.relu(F.conv2d(F.adaptive_avg_pool2d(h, 1), t[q + 'w1'], t[q + 'b1'])), t[q + 'w2'], t[q + 'b2']))
        return F.conv2d(h * s, t[q + 'wp'], t[q + 'bp']) + x

    @torch.no_grad()
    def forward(self, boards, valids):
        t, B = self.t, boards.shape[0]
        x = boards.reshape(B, 66, 5, 7).to(self.dtype)
        x1 = torch.einsum('oc,bcl->bol', t['1d.W0'], x[:, :6].permute(0, 3, 1, 2).flatten(2)) + t['1d.b0'][:, None]
        x1 = self._block1d('1d.0.', x1, False, False)
        pi = F.linear(self._block1d('1d.1.', x1, True, True).flatten(1), t['pi1d.W'], t['pi1d.b'])
        v = F.linear(self._block1d('1d.2.', x1, True, True).flatten(1), t['v1d.W'], t['v1d.b'])
        for m in range(self.n_mach):
            k = 'm%d.' % m
            xm = x[:, 6 + 10 * m:16 + 10 * m].flatten(1)[:, :343].reshape(B, 7, 7, 7).permute(0, 3, 1, 2)
            xm = F.conv2d(xm, t[k + 'c0'], padding=1)
            h = F.relu(F.conv2d(xm, t[k + 't.we'], t[k + 't.be']))
            h = F.relu(F.conv2d(h, t[k + 't.wd'], t[k + 't.bd'], padding=1, groups=h.shape[1]))
            xm = F.conv2d(h, t[k + 't.wp'], t[k + 't.bp']) + xm
            for hd in range(2):
                y = xm
                for b in range(3):
                    y = self._block2d(k + 'h%d.' % (3 * hd + b), y)
                if hd == 0:
                    pi = pi + F.linear(y.flatten(1), t['pi' + k + 'W'], t['pi' + k + 'b'])
                else:
                    v = v + F.linear(y.flatten(1), t['v' + k + 'W'], t['v' + k + 'b'])
        logits = F.linear(F.relu(F.linear(pi, t['f1.W'], t['f1.b'])), t['f2.W'], t['f2.b']).to(_wide(self.dtype))
        v = torch.tanh(F.linear(F.relu(F.linear(v, t['fv1.W'], t['fv1.b'])), t['fv2.W'], t['fv2.b']).to(_wide(self.dtype)))
        logits = torch.where(valids.bool(), logits, torch.full_like(logits, -1e8))
        return torch.softmax(logits, dim=1).contiguous(), v.contiguous()


class BotanikV1xHip(_EngineNet):
    """BotanikV1x (V10 or V11, A = 428) evaluated by the engine's one-launch kernel (azg_nn_bot_forward, csrc/nn_botanik.hip.h: the
    1-d branch on the vector ALUs, the machine branches' 1x1 convolutions and every policy Linear as f32 MFMA GEMMs, the depthwise 3x3 on
    the vector ALUs, final layers, masked softmax and tanh in the same launch).  Wraps a BotanikV1x; static pi / v buffers (HIP-graph
    capture of the engine's rounds)."""
    _FN, S = 'azg_nn_bot_forward', 2310
    MBLOB = 24496

    def __init__(self, base, max_batch=4096):
        from . import _lib
        self._lib, self.base, self.device = _lib, base, base.device
        self.P, self.A, self.n_mach = base.P, base.A, base.n_mach
        assert base.dtype == torch.float32 and self.device.type == 'cuda'
        self._keep = self.pack(base)
        self.ptrs = (C.c_void_p * 10)(*[t.data_ptr() for t in self._keep])
        self._alloc(max_batch)

    @staticmethod
    def frag(m, G, nct):
        """[K][N] -> [nct][G][64]: element m[G * (lane >> 4) + j][16 ct + (lane & 15)] (zero padded): the VGPR-resident fragments"""
        z = torch.zeros((4 * G, 16 * nct), dtype=torch.float32, device=m.device)
        z[:m.shape[0], :m.shape[1]] = m
        return z.view(4, G, nct, 16).permute(2, 1, 0, 3).contiguous().view(-1)

    @staticmethod
    def sfrag(m, KQ):
        """[K][N <= 432] -> [27][KQ][64]: element m[4 j + (lane >> 4)][16 ct + (lane & 15)] (zero padded): the streamed FC fragments"""
        z = torch.zeros((4 * KQ, 432), dtype=torch.float32, device=m.device)
        z[:m.shape[0], :m.shape[1]] = m
        return z.view(KQ, 4, 27, 16).permute(2, 0, 1, 3).contiguous().view(-1)

    @classmethod
    def pack(cls, base):
        """the 10 weight tensors of azg_nn_bot_forward (include/azg.h), on base's device"""
        t, d, M = base.t, base.device, range(base.n_mach)
        cat = lambda ts: torch.cat([x.reshape(-1) for x in ts]).contiguous()  # noqa: E731
        w1d = [t['1d.W0'], t['1d.b0']]
        for j in range(3):
            w1d += [t['1d.%d.%s' % (j, n)] for n in ('We', 'be', 'Wt', 'sd', 'bd', 'W1', 'b1', 'W2', 'b2', 'Wp', 'bp')]
        wm = []
        for m in M:
            k = 'm%d.' % m
            wm += [cls.frag(t[k + 'c0'].permute(2, 3, 1, 0).reshape(63, 16), 16, 1),
                   cls.frag(t[k + 't.we'].reshape(32, 16).t(), 4, 2), t[k + 't.be'], t[k + 't.wd'].reshape(32, 9).t(), t[k + 't.bd'],
                   cls.frag(t[k + 't.wp'].reshape(16, 32).t(), 8, 1), t[k + 't.bp']]
            for b in range(6):
                q = k + 'h%d.' % b
                wm += [cls.frag(t[q + 'we'].reshape(48, 16).t(), 4, 3), t[q + 'be'], t[q + 'wd'].reshape(48, 9).t(), t[q + 'bd'],
                       t[q + 'w1'].reshape(16, 48), t[q + 'b1'], t[q + 'w2'].reshape(48, 16), t[q + 'b2'],
                       cls.frag(t[q + 'wp'].reshape(16, 48).t(), 12, 1), t[q + 'bp']]
        wpi = [cls.sfrag(t['pi1d.W'].t(), 53)] + [cls.sfrag(t['pim%d.W' % m].t(), 196) for m in M]
        bpi = torch.zeros(432, dtype=torch.float32, device=d)
        bpi[:428] = t['pi1d.b'] + sum(t['pim%d.b' % m] for m in M)
        bf1, bf2 = torch.zeros(432, dtype=torch.float32, device=d), torch.zeros(432, dtype=torch.float32, device=d)
        bf1[:428], bf2[:428] = t['f1.b'], t['f2.b']
        tail = [t['v1d.b'] + sum(t['vm%d.b' % m] for m in M), t['fv1.W'], t['fv1.b'], t['fv2.W'], t['fv2.b']]
        keep = [cat(w1d), cat(wm), cat(wpi), bpi, cat([t['v1d.W']] + [t['vm%d.W' % m] for m in M]),
                cls.sfrag(t['f1.W'].t(), 108), bf1, cls.sfrag(t['f2.W'].t(), 108), bf2, cat(tail)]
        assert keep[0].numel() == 56 + 3 * 1629 and keep[1].numel() == cls.MBLOB * base.n_mach and keep[9].numel() == 14
        return keep

    def _ints(self):
        return (self.n_mach, self.P, self.A)


class TorchModuleEvaluator:
    """Leaf evaluator around ANY torch module with the reference's forward signature
    `module(board f32[B, *board_shape], valid_actions bool[B, A]) -> (log_pi f32[B, A], v f32[B, P])` -- the torch branch of
    GenericNNetWrapper.predict (:111-120) batched on PyTorch-ROCm.  It is the evaluator of the games whose nets have no engine
    kernel: the six f4 games with the reference's own `<G>NNet` modules (import them from the reference, load their checkpoints
    as usual) or a user's architecture.  Same `predict_batch` contract as the engine-kernel nets, so SelfPlayEngine / BatchedMCTS /
    BatchedArena / Coach take it unchanged (HIP-graph capture included: the module runs inside the captured round)."""

    def __init__(self, module, game, max_batch=None):
        self.module = module.to(game.device).eval()
        self.shape = tuple(game.getBoardSize())
        self.device = game.device

    def predict_batch(self, boards, valids):
        with torch.no_grad():
            b = boards.reshape((boards.shape[0],) + self.shape).to(torch.float32)
            log_pi, v = self.module(b, valids.bool())
            return torch.exp(log_pi).to(torch.float32).contiguous(), v.to(torch.float32).contiguous()

    def clone_buffers(self):
        return self


class RolloutEvaluator:
    """Leaf evaluator WITHOUT a net -- the pure-MCTS contestant, and the way to search a game that has no checkpoint yet: a uniform prior
    over the valid moves, and as the value of a leaf the mean result of `n_playouts` uniformly random playouts from it, all of a batch in
    one launch of azg_env_playouts (csrc/playout.hip.h).  The leaves are canonical (the player to move is seat 0) and the playouts'
    results are in the seat numbering of the board they start from, so v[t, 0] is the leaf player's own expected result: NeuralNet.predict's
    v (MCTS.py:131,153,175-178).  Same `predict_batch` contract as the engine nets, so BatchedMCTS / MCTS / BatchedArena / SelfPlayEngine
    take it wherever they take an nnet (on the two-kernel rounds: it is no pipeline net).

    Playout j of batch row t draws from stream stream0 + t * n_playouts + j at counters[t * n_playouts + j]; the kernel advances the
    counters, so every call -- a replay of a captured round too -- plays fresh games.  Rows whose `valids` row is empty (the leaf rows a
    round never wrote) run nothing: pi and v are zero and their counters stay."""

    _BLOCK = 1 << 32                      # streams between an evaluator and its clone_buffers() copies

    def __init__(self, game, n_playouts=8, max_plies=4096, stream0=1 << 40, max_batch=1):
        if int(n_playouts) < 1 or not 1 <= int(max_plies) <= 65535:
            raise ValueError('RolloutEvaluator: n_playouts >= 1 and 1 <= max_plies <= 65535')
        self.game, self.device = game, game.device
        self.k, self.max_plies, self.stream0 = int(n_playouts), int(max_plies), int(stream0)
        self.S, self.A, self.P = game.S, game.A, game.P
        self._family = [int(stream0), 0]  # shared by the clones: the first evaluator's stream0, clones handed out so far
        self.counters = torch.zeros(0, dtype=torch.int64, device=self.device)
        self._alloc(max(1, int(max_batch)))

    def _alloc(self, B):
        dev, k, old = self.device, self.k, self.counters
        self.maxB = B
        self.pi = torch.zeros((B, self.A), dtype=torch.float32, device=dev)
        self.v = torch.zeros((B, self.P), dtype=torch.float32, device=dev)
        self.ended = torch.zeros((B, k, self.P), dtype=torch.float32, device=dev)
        self.plies = torch.zeros((B, k), dtype=torch.int32, device=dev)
        self.status = torch.zeros((B, k), dtype=torch.uint8, device=dev)
        self.active = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.counters = torch.zeros(B * k, dtype=torch.int64, device=dev)
        n = min(old.numel(), B * k)
        self.counters[:n] = old[:n]       # (a larger batch keeps the streams it already drew from where they are)

    def clone_buffers(self):
        """an evaluator with its own buffers and counters on a stream block of its own (concurrent groups never share a stream)"""
        other = copy.copy(self)
        self._family[1] += 1
        other.stream0 = self._family[0] + self._family[1] * self._BLOCK
        other.counters = torch.zeros(0, dtype=torch.int64, device=self.device)
        other._alloc(self.maxB)
        return other

    @torch.no_grad()
    def predict_batch(self, boards, valids):
        from .games import playouts_into
        B = boards.shape[0]
        if B > self.maxB:
            self._alloc(B)
        boards = boards.reshape(B, -1)
        va = valids.to(torch.float32)
        assert va.shape == (B, self.A) and va.is_cuda
        cnt = va.sum(dim=1, keepdim=True)
        pi, v, active = self.pi[:B], self.v[:B], self.active[:B]
        torch.div(va, cnt.clamp(min=1.0), out=pi)
        active.copy_(cnt[:, 0] != 0)
        playouts_into(self.game, boards, None, self.k, self.max_plies, active, self.stream0, self.counters[:B * self.k],
                      self.ended[:B], self.plies[:B], self.status[:B])
        torch.mean(self.ended[:B], dim=1, out=v)
        v.mul_(active[:, None])           # (an idle row's playout results are whatever an earlier call left there)
        return pi, v

    def predict(self, board, valid_actions):
        b = torch.as_tensor(np.asarray(board, dtype=np.int8)).reshape(1, -1).to(self.device)
        va = torch.as_tensor(np.asarray(valid_actions).astype(np.uint8)).reshape(1, -1).to(self.device)
        pi, v = self.predict_batch(b, va)
        return pi[0].cpu().numpy(), v[0].cpu().numpy()


def eval_losses(pi, v, target_pi, z, q, q_weight, active=None, totals=None, accumulate=False):
    """azg_eval_losses (include/azg.h; csrc/loss.hip.h) on CUDA tensors: the validation losses of B examples from a net's outputs.  pi
    f32[B, A] PROBABILITIES as predict_batch returns them, v f32[B, P], target_pi f32[B, A], z / q f32[B, P], active u8 / bool[B] or None.
    -> (rows f64[B, 2]: the row's KL sum and its squared value error, flags int32[B, 2]: top-1 agreement and the number of actions whose
    probability was below FLT_MIN and was floored there, totals f64[4]: the sums of the four columns over the active rows).  With
    accumulate=True the sums are added to what `totals` holds (a validation set in chunks: one host read at the end).  rows and flags are
    allocated here: the C call owns no memory.  One call = two launches on the current stream, nothing synchronised."""
    B, A = pi.shape
    P = v.shape[1]
    for x, shape in ((pi, (B, A)), (target_pi, (B, A)), (v, (B, P)), (z, (B, P)), (q, (B, P))):
        assert x.dtype == torch.float32 and tuple(x.shape) == shape and x.is_contiguous() and x.device == pi.device, \
            'eval_losses: dtype / shape / layout of an argument'
    assert active is None or (active.dtype in (torch.uint8, torch.bool) and active.shape == (B,) and active.is_contiguous()
                              and active.device == pi.device), 'eval_losses: dtype / shape / layout of active'
    if totals is None:
        assert not accumulate, 'eval_losses: accumulate=True needs the totals to add to'
        totals = torch.zeros(4, dtype=torch.float64, device=pi.device)
    assert totals.dtype == torch.float64 and totals.shape == (4,) and totals.is_contiguous() and totals.device == pi.device
    rows = torch.empty((B, 2), dtype=torch.float64, device=pi.device)
    flags = torch.empty((B, 2), dtype=torch.int32, device=pi.device)
    from . import _lib
    _lib.check(_lib.lib().azg_eval_losses(_ptr(pi), _ptr(v), _ptr(target_pi), _ptr(z), _ptr(q), _ptr(active) if active is not None else None,
                                          B, A, P, C.c_float(float(q_weight)), _ptr(rows), _ptr(flags), _ptr(totals),
                                          1 if accumulate else 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return rows, flags, totals


def evaluate_examples(evaluator, cols, q_weight, batch=4096):
    """The validation losses of GenericNNetWrapper.evaluate (:159-177) for any evaluator with predict_batch (an engine net, a
    TorchModuleEvaluator, a RolloutEvaluator): cols = (boards int8[n, S], pi f32[n, A], z f32[n, P], valids u8 / bool[n, A], q f32[n, P])
    tensors or arrays as train.train takes them.  Chunks of `batch` rows go through predict_batch and eval_losses(accumulate=True); one
    device-to-host read at the end.  -> dict(loss_pi = KL total / n ('batchmean'), loss_v = squared error total / (n P), top1 = the
    fraction of rows whose policy argmax is the target's, floored = the number of floored probabilities (see eval_losses), n)"""
    dev = getattr(evaluator, 'device', None) or 'cuda:0'
    boards, pi, z, valids, q = [torch.as_tensor(x).to(dev) for x in cols[:5]]
    n = int(boards.shape[0])
    boards = boards.reshape(n, -1).to(torch.int8).contiguous()
    valids = valids.reshape(n, -1).to(torch.uint8).contiguous()
    pi, z, q = (x.reshape(n, -1).to(torch.float32).contiguous() for x in (pi, z, q))
    P = int(z.shape[1])
    totals = torch.zeros(4, dtype=torch.float64, device=boards.device)
    for a in range(0, n, int(batch)):
        b = min(n, a + int(batch))
        out_pi, out_v = evaluator.predict_batch(boards[a:b], valids[a:b])
        eval_losses(out_pi.contiguous(), out_v.contiguous(), pi[a:b], z[a:b], q[a:b], q_weight, totals=totals, accumulate=True)
    t = totals.cpu().tolist()
    d = max(n, 1)
    return dict(loss_pi=t[0] / d, loss_v=t[1] / (d * P), top1=t[2] / d, floored=int(t[3]), n=n)
