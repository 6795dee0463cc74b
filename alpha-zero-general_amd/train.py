"""Next-row f1: the trainer side of Coach.learn on PyTorch-ROCm autograd.

`SplendorV80Module` is a trainable nn.Module with the reference's parameter names (splendor/SplendorNNet.py:148-202,
262-283,397-440), so `state_dict()` round-trips with the reference's checkpoints and with the inference nets of
azg_amd.nnet (which fold its BatchNorms).  `train()` is GenericNNetWrapper.train (:44-92): AdamW + OneCycleLR,
loss = KLDiv(pi) + 0.25 * MSE((z + q_weight*q) / (1 + q_weight)) (:179-190), batches sampled without replacement inside a
batch, `epochs * (len(examples) // batch_size)` steps."""
import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


class _LinearNormAct(nn.Module):
    """Linear over the channel axis (or over the token axis when depthwise) of x[B, C, L] + BatchNorm1d(C) + activation"""

    def __init__(self, n_in, n_out, act, depthwise=False, channels=None):
        super().__init__()
        self.linear = nn.Linear(n_in, n_out, bias=False)
        self.norm = nn.BatchNorm1d(channels if depthwise else n_out)
        self.activation = act() if act is not None else nn.Identity()
        self.depthwise = depthwise

    def forward(self, x):
        y = self.linear(x) if self.depthwise else self.linear(x.transpose(1, 2)).transpose(1, 2)
        return self.activation(self.norm(y))


class _SE(nn.Module):
    def __init__(self, channels, squeeze, setype):
        super().__init__()
        self.setype = setype
        self.fc1, self.fc2 = nn.Linear(channels, squeeze), nn.Linear(squeeze, channels)

    def forward(self, x):
        s = x.mean(dim=2) if self.setype == 'avg' else x.amax(dim=2)
        s = F.hardsigmoid(self.fc2(F.relu(self.fc1(s))))
        return x * s[:, :, None]


def _make_divisible(v, divisor=8, min_value=None):
    """torchvision.models._utils._make_divisible (the SE squeeze width of the reference blocks)"""
    min_value = divisor if min_value is None else min_value
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    return new_v + divisor if new_v < 0.9 * v else new_v


class _Block(nn.Module):
    """InvertedResidual1d (SplendorNNet.py:189-202, AzulNNet.py:47-80): residual only when in == out channels"""

    def __init__(self, c, e, use_hs, setype, tokens=7, c_out=None):
        super().__init__()
        c_out = c if c_out is None else c_out
        act = nn.Hardswish if use_hs else nn.ReLU
        self.expand = _LinearNormAct(c, e, act)
        self.depthwise = _LinearNormAct(tokens, tokens, act, depthwise=True, channels=e)
        self.se = _SE(e, _make_divisible(e // 4, 8), setype)
        self.project = _LinearNormAct(e, c_out, None)
        self.use_res_connect = c == c_out

    def forward(self, x):
        y = self.project(self.se(self.depthwise(self.expand(x))))
        return y + x if self.use_res_connect else y


class _MobileNet1dModule(nn.Module):
    """The reference's one-trunk-block MobileNetV3-1d nets with its parameter names: [B, C, L] boards (no transpose), first_layer, ONE
    trunk block C -> E -> C (ReLU, mean squeeze), policy / value head blocks C -> E -> C (Hardswish, max squeeze) + Flatten + Linear +
    ReLU + Linear, dropout after the trunk in training mode (splendor/SplendorNNet.py:397-440, MinivillesNNet.py:101-123,166-172,
    TLPNNet.py:175-217)"""

    def __init__(self, C, L, E, num_players, action_size, dropout):
        super().__init__()
        self.C, self.L, self.P, self.A, self.dropout = C, L, num_players, action_size, dropout
        self.first_layer = _LinearNormAct(C, C, None)
        self.trunk = nn.Sequential(_Block(C, E, False, 'avg', tokens=L))
        self.output_layers_PI = nn.Sequential(_Block(C, E, True, 'max', tokens=L), nn.Flatten(1), nn.Linear(L * C, action_size), nn.ReLU(),
                                              nn.Linear(action_size, action_size))
        self.output_layers_V = nn.Sequential(_Block(C, E, True, 'max', tokens=L), nn.Flatten(1), nn.Linear(L * C, num_players), nn.ReLU(),
                                             nn.Linear(num_players, num_players))
        self.register_buffer('lowvalue', torch.FloatTensor([-1e8]))

    def forward(self, boards, valid_actions):
        """-> (log pi [B, A], v [B, P]) like the reference module"""
        x = boards.reshape(-1, self.C, self.L).float()
        x = self.first_layer(x)
        x = F.dropout(self.trunk(x), p=self.dropout, training=self.training)
        v = self.output_layers_V(x)
        pi = torch.where(valid_actions.bool(), self.output_layers_PI(x), self.lowvalue)
        return F.log_softmax(pi, dim=1), torch.tanh(v)


class SplendorV80Module(_MobileNet1dModule):
    version = 80

    def __init__(self, num_players=2, action_size=81, dropout=0.0):
        C = 32 + 10 * num_players + num_players * num_players
        super().__init__(C, 7, 3 * C, num_players, action_size, dropout)


class MinivillesV82Module(_MobileNet1dModule):
    """minivilles/MinivillesNNet.py nn_version 82 (:101-123,166-172): [B, C, 2] boards with C = 18 + 20 P (58 / 78 / 98 for the
    shipped 2 / 3 / 4-player checkpoints), blocks C -> 3C -> C"""
    version = 82

    def __init__(self, num_players=2, action_size=21, dropout=0.0):
        C = 18 + 20 * num_players
        super().__init__(C, 2, 3 * C, num_players, action_size, dropout)


class TLPV83Module(_MobileNet1dModule):
    """thelittleprince/TLPNNet.py nn_version 83 (:175-217): [B, C, 15] boards with C = 1 + 18 P (55 / 73 / 91 for the shipped
    3 / 4 / 5-player checkpoints), blocks C -> int(1.5 C) -> C"""
    version = 83

    def __init__(self, num_players=3, action_size=9, dropout=0.0):
        C = 1 + 18 * num_players
        super().__init__(C, 15, int(1.5 * C), num_players, action_size, dropout)


class AzulV84Module(nn.Module):
    """azul/AzulNNet.py nn_version 84 (:91-113,130-142) with the reference's parameter names: [B, 23, 6] boards, trunk block
    23->115->23, policy head block 23->115->46 (no residual) + Linear(276,180)+ReLU+Linear, value head block 23->46->23."""
    version = 84

    def __init__(self, num_players=2, action_size=180, dropout=0.0):
        super().__init__()
        self.C, self.L, self.P, self.A, self.dropout = 23, 6, num_players, action_size, dropout
        C, L = self.C, self.L
        self.first_layer = _LinearNormAct(C, C, None)
        self.trunk = nn.Sequential(_Block(C, 5 * C, False, 'avg', tokens=L))
        self.output_layers_PI = nn.Sequential(_Block(C, 5 * C, True, 'avg', tokens=L, c_out=2 * C), nn.Flatten(1),
                                              nn.Linear(2 * C * L, action_size), nn.ReLU(), nn.Linear(action_size, action_size))
        self.output_layers_V = nn.Sequential(_Block(C, 2 * C, True, 'avg', tokens=L), nn.Flatten(1), nn.Linear(C * L, num_players),
                                             nn.ReLU(), nn.Linear(num_players, num_players))
        self.register_buffer('lowvalue', torch.FloatTensor([-1e8]))

    def forward(self, boards, valid_actions):
        x = boards.reshape(-1, self.C, self.L).float()
        x = self.first_layer(x)
        x = F.dropout(self.trunk(x), p=self.dropout, training=self.training)
        v = self.output_layers_V(x)
        pi = torch.where(valid_actions.bool(), self.output_layers_PI(x), self.lowvalue)
        return F.log_softmax(pi, dim=1), torch.tanh(v)


class _ResBlock(nn.Module):
    """SimpleResBlock (santorini/SantoriniNNet.py:71-84): conv3x3+BN+ReLU, conv3x3+BN, + input, ReLU"""

    def __init__(self, c):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(c, c, 3, padding=1, bias=False), nn.BatchNorm2d(c)
        self.conv2, self.bn2 = nn.Conv2d(c, c, 3, padding=1, bias=False), nn.BatchNorm2d(c)

    def forward(self, x):
        y = F.relu(self.bn1(self.conv1(x)))
        return F.relu(self.bn2(self.conv2(y)) + x)


class _Head2d(nn.Module):
    """SimpleHead / HeadWithMeta (SantoriniNNet.py:17-69): 1x1 bottleneck conv + BN + ReLU, flatten (+ the 32 metadata
    features), Linear (policy) or Linear + ReLU + Linear (value)"""

    def __init__(self, c, bottleneck, out, value, meta=0):
        super().__init__()
        self.conv1x1, self.bn, self.value = nn.Conv2d(c, bottleneck, 1, bias=False), nn.BatchNorm2d(bottleneck), value
        flat = bottleneck * 25 + meta
        if value:
            self.fc1, self.fc2 = nn.Linear(flat, 64), nn.Linear(64, out)
        else:
            self.fc = nn.Linear(flat, out)

    def forward(self, x, meta=None):
        x = torch.flatten(F.relu(self.bn(self.conv1x1(x))), 1)
        if meta is not None:
            x = torch.cat([x, meta], dim=1)
        return self.fc2(F.relu(self.fc1(x))) if self.value else self.fc(x)


class SantoriniV89Module(nn.Module):
    """santorini/SantoriniNNet.py nn_version 89 (:194-219,273-281; no gods, A = 162) with the reference's parameter names:
    conv3x3(2->64)+BN+ReLU, five SimpleResBlocks, SimpleHead heads (bottlenecks 2 / 1)."""
    version = 89

    def __init__(self, num_players=2, action_size=162, dropout=0.0):
        super().__init__()
        self.P, self.A, self.dropout = num_players, action_size, dropout
        self.first_layer = nn.Sequential(nn.Conv2d(2, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU())
        self.trunk = nn.Sequential(*[_ResBlock(64) for _ in range(5)])
        self.head_PI, self.head_V = _Head2d(64, 2, action_size, False), _Head2d(64, 1, num_players, True)
        self.register_buffer('lowvalue', torch.FloatTensor([-1e8]))

    def forward(self, boards, valid_actions):
        x = boards.reshape(-1, 5, 5, 3).float().permute(0, 3, 1, 2)
        f = self.trunk(self.first_layer(x[:, :2]))
        v = self.head_V(f)
        pi = torch.where(valid_actions.bool(), self.head_PI(f), self.lowvalue)
        return F.log_softmax(pi, dim=1), torch.tanh(v)


class _MBBlock2d(nn.Module):
    """torchvision's MobileNetV3 InvertedResidual as the reference configures it (SantoriniNNet.py:172-178: 64 -> 192 -> 64,
    3x3 depthwise, no SE, ReLU, residual); parameter names block.{0,1,2}.{0 conv, 1 BatchNorm}"""

    def __init__(self, c, e):
        super().__init__()
        cna = lambda i, o, k, g, act: nn.Sequential(nn.Conv2d(i, o, k, padding=(k - 1) // 2, groups=g, bias=False),  # noqa: E731
                                                    nn.BatchNorm2d(o), *([nn.ReLU()] if act else []))
        self.block = nn.Sequential(cna(c, e, 1, 1, True), cna(e, e, 3, e, True), cna(e, c, 1, 1, False))

    def forward(self, x):
        return self.block(x) + x


class SantoriniV78Module(nn.Module):
    """santorini/SantoriniNNet.py nn_version 78 (:167-192,264-271; with gods, A = 1782) with the reference's parameter names:
    conv3x3(2->64), ten InvertedResidual blocks, meta_fc (gods plane -> 32 features), HeadWithMeta heads (bottlenecks 4 / 2)."""
    version = 78

    def __init__(self, num_players=2, action_size=1782, dropout=0.0):
        super().__init__()
        self.P, self.A, self.dropout = num_players, action_size, dropout
        self.first_layer = nn.Conv2d(2, 64, 3, padding=1, bias=False)
        self.trunk = nn.Sequential(*[_MBBlock2d(64, 192) for _ in range(10)])
        self.meta_fc = nn.Sequential(nn.Flatten(1), nn.Linear(25, 32), nn.ReLU())
        self.head_PI, self.head_V = _Head2d(64, 4, action_size, False, meta=32), _Head2d(64, 2, num_players, True, meta=32)
        self.register_buffer('lowvalue', torch.FloatTensor([-1e8]))

    def forward(self, boards, valid_actions):
        x = boards.reshape(-1, 5, 5, 3).float().permute(0, 3, 1, 2)
        f = self.trunk(self.first_layer(x[:, :2]))
        meta = self.meta_fc(x[:, 2:3])
        v = self.head_V(f, meta)
        pi = torch.where(valid_actions.bool(), self.head_PI(f, meta), self.lowvalue)
        return F.log_softmax(pi, dim=1), torch.tanh(v)

class AbaloneV21Module(nn.Module):
    """abalone/AbaloneNNet.py nn_version 21 (:120-160, forward :173-201; Belgian Daisy, A = 3402) with the reference's parameter
    names: conv3x3(3->24)+BN+ReLU, four InvertedResidual blocks 24 -> 48 -> 24, meta_fc (6 metadata values -> 16), policy 1x1
    conv 24->42 + BN, value 1x1 conv 24->4 + BN + ReLU -> Linear(340, 64) + ReLU -> Linear(64, P)."""
    version = 21

    def __init__(self, num_players=2, action_size=3402, dropout=0.0):
        super().__init__()
        self.P, self.A, self.dropout = num_players, action_size, dropout
        self.first_layer = nn.Sequential(nn.Conv2d(3, 24, 3, padding=1, bias=False), nn.BatchNorm2d(24), nn.ReLU())
        self.trunk = nn.Sequential(*[_MBBlock2d(24, 48) for _ in range(4)])
        self.meta_fc = nn.Sequential(nn.Linear(6, 16), nn.ReLU())
        self.head_PI = nn.Sequential(nn.Conv2d(24, action_size // 81, 1, bias=False), nn.BatchNorm2d(action_size // 81))
        self.head_V_conv = nn.Sequential(nn.Conv2d(24, 4, 1, bias=False), nn.BatchNorm2d(4), nn.ReLU())
        self.head_V_fc = nn.Sequential(nn.Linear(4 * 81 + 16, 64), nn.ReLU(), nn.Linear(64, num_players))
        self.register_buffer('lowvalue', torch.FloatTensor([-1e8]))

    def forward(self, boards, valid_actions):
        x = boards.reshape(-1, 9, 9, 4).float()
        meta = self.meta_fc(x[:, 0, 0:6, 3])
        f = self.trunk(self.first_layer(x[..., :3].permute(0, 3, 1, 2)))
        pi = self.head_PI(f).permute(0, 2, 3, 1).flatten(1)
        v = self.head_V_fc(torch.cat([torch.flatten(self.head_V_conv(f), 1), meta], dim=1))
        pi = torch.where(valid_actions.bool(), pi, self.lowvalue)
        return F.log_softmax(pi, dim=1), torch.tanh(v)

class _SmallworldStem(nn.Module):
    """smallworld/SmallworldNNet.py InputStem (:86-137) with its parameter names: embeddings of the clamped columns 1, 2, 7, a 5 -> D
    projection of columns 0, 3..6 / 10, a 16 -> D projection of the 8 low bits of columns 3 and 4, out_proj over the five parts, LayerNorm"""

    def __init__(self, d):
        super().__init__()
        self.emb_ppl, self.emb_pwr, self.emb_player = nn.Embedding(31, d), nn.Embedding(41, d), nn.Embedding(6, d)
        self.num_proj, self.bit_proj = nn.Linear(5, d), nn.Linear(16, d)
        self.out_proj, self.norm = nn.Linear(5 * d, d), nn.LayerNorm(d)
        self.register_buffer('powers_of_2', 2 ** torch.arange(8, dtype=torch.long))

    def forward(self, x):
        c = x.long()
        e = [self.emb_ppl((c[..., 1] + 15).clamp(0, 30)), self.emb_pwr((c[..., 2] + 20).clamp(0, 40)), self.emb_player((c[..., 7] + 1).clamp(0, 5))]
        e.append(self.num_proj(torch.cat([x[..., 0:1], x[..., 3:7]], dim=-1).float() / 10.0))
        bits = torch.cat([torch.div(c[..., j:j + 1], self.powers_of_2, rounding_mode='floor') % 2 for j in (3, 4)], dim=-1)
        e.append(self.bit_proj(bits.float()))
        return self.norm(self.out_proj(torch.cat(e, dim=-1)))


class _SmallworldHead(nn.Module):
    """ActionSlicerHead (:139-180): local 48 -> 5 on the nA area tokens, mean of the rest -> global 48 -> 16 and value 48 -> P, in the
    policy layout [l0 | l1 | l2 | l3 | g0..7 | l4 | g8..15]"""

    def __init__(self, d, action_size, num_players):
        super().__init__()
        self.nb_areas = (action_size - 16) // 5
        self.local_head, self.global_head, self.value_head = nn.Linear(d, 5), nn.Linear(d, 16), nn.Linear(d, num_players)

    def forward(self, x):
        loc = self.local_head(x[:, :self.nb_areas])
        g = x[:, self.nb_areas:].mean(dim=1)
        gl = self.global_head(g)
        pi = torch.cat([loc[..., 0], loc[..., 1], loc[..., 2], loc[..., 3], gl[:, :8], loc[..., 4], gl[:, 8:]], dim=1)
        return pi, self.value_head(g)


class SmallworldV62Module(nn.Module):
    """smallworld/SmallworldNNet.py nn_version 62 (:246-254, forward :268-294; pretrained_{2,3,4}pl.pt) with the reference's parameter and
    buffer names: stem.*, three nn.TransformerEncoderLayer (d_model 48, 3 heads, feed-forward 192, post-norm) as trunk.layers.N.*, head.*,
    lowvalue.  In training mode the stem output goes through dropout when dropout > 0, and the encoder layers apply their own dropouts."""
    version = 62
    N_TOKENS = {2: 40, 3: 52, 4: 66}

    def __init__(self, num_players=2, action_size=131, dropout=0.0):
        super().__init__()
        self.P, self.A, self.dropout, self.N = num_players, action_size, dropout, self.N_TOKENS[num_players]
        self.stem = _SmallworldStem(48)
        self.head = _SmallworldHead(48, action_size, num_players)
        layer = nn.TransformerEncoderLayer(d_model=48, nhead=3, dim_feedforward=192, dropout=dropout, batch_first=True)
        self.trunk = nn.TransformerEncoder(layer, num_layers=3, enable_nested_tensor=False)
        self.register_buffer('lowvalue', torch.FloatTensor([-1e8]))

    def forward(self, boards, valid_actions):
        x = self.stem(boards.reshape(-1, self.N, 8))
        if self.training and self.dropout > 0:
            x = F.dropout(x, p=self.dropout)
        pi, v = self.head(self.trunk(x))
        pi = torch.where(valid_actions.bool(), pi, self.lowvalue)
        return F.log_softmax(pi, dim=1), torch.tanh(v)

class _SqueezeExcitation2d(nn.Module):
    """torchvision's SqueezeExcitation: mean over the cells, fc1 (1x1 conv) + ReLU, fc2 (1x1 conv) + Hardsigmoid, scale"""

    def __init__(self, c, squeeze):
        super().__init__()
        self.fc1, self.fc2 = nn.Conv2d(c, squeeze, 1), nn.Conv2d(squeeze, c, 1)

    def forward(self, x):
        return x * F.hardsigmoid(self.fc2(F.relu(self.fc1(F.adaptive_avg_pool2d(x, 1)))))


class _MBBlockSE1x1(nn.Module):
    """torchvision's MobileNetV3 InvertedResidual with kernel 1, SE and Hardswish, as AkropolisNNet.py:136 configures `proj_p`
    (8P + 24 -> 32 -> 16): expand 1x1 + BN + Hardswish, depthwise 1x1 + BN + Hardswish, SE (squeeze 8), project 1x1 + BN; the residual
    only when in == out channels.  Parameter names block.{0,1,3}.{0 conv, 1 BatchNorm}, block.2.fc{1,2}"""

    def __init__(self, c_in, e, c_out):
        super().__init__()
        cna = lambda i, o, g, act: nn.Sequential(nn.Conv2d(i, o, 1, groups=g, bias=False), nn.BatchNorm2d(o),  # noqa: E731
                                                 *([nn.Hardswish()] if act else []))
        self.block = nn.Sequential(cna(c_in, e, 1, True), cna(e, e, e, True), _SqueezeExcitation2d(e, _make_divisible(e // 4, 8)),
                                   cna(e, c_out, 1, False))
        self.use_res_connect = c_in == c_out

    def forward(self, x):
        y = self.block(x)
        return y + x if self.use_res_connect else y


class AkropolisV31Module(nn.Module):
    """akropolis/AkropolisNNet.py nn_version 31 (constructor :91-146, forward :377-388,573-622; pretrained_{2,3,4}pl.pt) with the
    reference's parameter names: embed, conv1d_constr, dense_scores, conv2d_boards, dense_globs, final_layers_V, proj_i, proj_p, proj_o,
    b1n, lowvalue.  In training mode s1, g1 and the conv1d output go through dropout, as in the reference."""
    version = 31

    def __init__(self, num_players=2, action_size=4056, dropout=0.0):
        super().__init__()
        P = num_players
        self.P, self.A, self.dropout, self.CS = P, action_size, dropout, P + 2
        D, T, S, G, B, r = 3, 32, 16, 8, 8, 16
        self.embed = nn.Embedding(12, D)
        self.conv1d_constr = nn.Sequential(nn.Conv1d(D, T, kernel_size=3), nn.Hardswish())
        self.dense_scores = nn.Sequential(nn.Linear(15 * P, S))
        self.conv2d_boards = nn.Sequential(nn.Conv2d(D + 2, B, 3, padding=1), nn.BatchNorm2d(B), nn.Hardswish(),
                                           nn.Conv2d(B, B, 3, padding=1), nn.BatchNorm2d(B), nn.Hardswish())
        self.dense_globs = nn.Sequential(nn.Linear(2, G), nn.BatchNorm1d(G), nn.Hardswish())
        self.final_layers_V = nn.Sequential(nn.Flatten(1), nn.Linear(self.CS * (T + S + G), r), nn.BatchNorm1d(r), nn.Hardswish(),
                                            nn.Linear(r, r), nn.Hardswish(), nn.Linear(r, P))
        self.proj_i = nn.Linear(T + S + G, r)
        self.proj_p = nn.Sequential(_MBBlockSE1x1(P * B + G + S, 2 * r, r))
        self.proj_o = nn.Linear(T + G + S, 6 * r)
        self.b1n = nn.Sequential(nn.BatchNorm1d(r), nn.Hardswish())
        self.register_buffer('lowvalue', torch.FloatTensor([-1e8]))

    def forward(self, boards, valid_actions):
        P, CS = self.P, self.CS
        x = boards.reshape(-1, 13, 13, 3 * P + 2).float().permute(0, 3, 1, 2)
        N = x.shape[0]
        drop = lambda t: F.dropout(t, p=self.dropout, training=self.training)  # noqa: E731
        s1 = drop(self.dense_scores(x[:, 3 * P, :3 * P, :5].flatten(1)))
        g1 = drop(self.dense_globs(x[:, 3 * P + 1, CS + 1, :2]))
        descr = self.embed(x[:, :P].clamp(0, 11).long())                                  # N, P, 13, 13, D
        bx = torch.cat([descr, x[:, P:2 * P, ..., None], x[:, 2 * P:3 * P, ..., None]], dim=-1)
        bf = [self.conv2d_boards(bx[:, i].permute(0, 3, 1, 2)) for i in range(P)]
        fused_4d = torch.cat(bf + [s1[..., None, None].expand(-1, -1, 13, 13), g1[..., None, None].expand(-1, -1, 13, 13)], dim=1)
        ce = self.embed(x[:, 3 * P + 1, :CS, :3].clamp(0, 11).long())                      # N, CS, 3, D
        t = drop(self.conv1d_constr(ce.flatten(0, 1).permute(0, 2, 1))).view(N, CS, -1)
        f3 = torch.cat([t, s1[:, None].expand(-1, CS, -1), g1[:, None].expand(-1, CS, -1)], dim=-1)
        a = self.b1n(self.proj_i(f3).permute(0, 2, 1)).permute(0, 2, 1)                  # N, CS, r
        p = self.proj_p(fused_4d).flatten(2)                                                # N, r, 169
        h = self.proj_o(f3).view(N, CS, 6, -1)                                              # N, CS, 6, r
        pi = torch.einsum('nrk,ncor->ncko', p, a[:, :, None] * h).flatten(1)                # (the reference's 6-d product, summed over r)
        pi = torch.where(valid_actions.bool(), pi, self.lowvalue)
        v = self.final_layers_V(f3)
        return F.log_softmax(pi, dim=1), torch.tanh(v)


class _MBBlock2dSE(nn.Module):
    """torchvision's MobileNetV3 InvertedResidual with a 3x3 depthwise, SE and Hardswish, as BotanikNNet.py:127-137 configures the head
    blocks (16 -> 48 -> 16, squeeze 16, residual).  Parameter names block.{0,1,3}.{0 conv, 1 BatchNorm}, block.2.fc{1,2}"""

    def __init__(self, c, e):
        super().__init__()
        cna = lambda i, o, k, g, act: nn.Sequential(nn.Conv2d(i, o, k, padding=(k - 1) // 2, groups=g, bias=False),  # noqa: E731
                                                    nn.BatchNorm2d(o), *([nn.Hardswish()] if act else []))
        self.block = nn.Sequential(cna(c, e, 1, 1, True), cna(e, e, 3, e, True), _SqueezeExcitation2d(e, _make_divisible(e // 4, 8)),
                                   cna(e, c, 1, 1, False))

    def forward(self, x):
        return self.block(x) + x


class BotanikV10Module(nn.Module):
    """botanik/BotanikNNet.py nn_version 10 (:105-160, forward :251-273) with the reference's parameter names: the 1-d branch
    (first_layer_1d, trunk_1d, output_layers_{PI,V}_1d) on rows 0..5 and one machine branch (first_layer_mach0, trunk_mach0,
    output_layers_{PI,V}_mach0) on rows 6..15, summed into final_layers_PI / final_layers_V.  In training mode the trunk_1d output goes
    through dropout, as in the reference (:256)."""
    version = 10
    N_MACH = 1

    def __init__(self, num_players=2, action_size=428, dropout=0.0):
        super().__init__()
        self.P, self.A, self.dropout = num_players, action_size, dropout
        self.first_layer_1d = _LinearNormAct(7, 7, None)
        self.trunk_1d = nn.Sequential(_Block(7, 21, False, 'avg', tokens=30))
        self.output_layers_PI_1d = nn.Sequential(_Block(7, 21, True, 'max', tokens=30), nn.Flatten(1), nn.Linear(210, action_size))
        self.output_layers_V_1d = nn.Sequential(_Block(7, 21, True, 'max', tokens=30), nn.Flatten(1), nn.Linear(210, num_players))
        for m in range(self.N_MACH):
            setattr(self, 'first_layer_mach%d' % m, nn.Conv2d(7, 16, 3, padding=1, bias=False))
            setattr(self, 'trunk_mach%d' % m, nn.Sequential(_MBBlock2d(16, 32)))
            setattr(self, 'output_layers_PI_mach%d' % m, nn.Sequential(*[_MBBlock2dSE(16, 48) for _ in range(3)], nn.Flatten(1),
                                                                      nn.Linear(784, action_size)))
            setattr(self, 'output_layers_V_mach%d' % m, nn.Sequential(*[_MBBlock2dSE(16, 48) for _ in range(3)], nn.Flatten(1),
                                                                     nn.Linear(784, num_players)))
        self.final_layers_PI = nn.Sequential(nn.Linear(action_size, action_size), nn.ReLU(), nn.Linear(action_size, action_size))
        self.final_layers_V = nn.Sequential(nn.Linear(num_players, num_players), nn.ReLU(), nn.Linear(num_players, num_players))
        self.register_buffer('lowvalue', torch.FloatTensor([-1e8]))

    def forward(self, boards, valid_actions):
        x = boards.reshape(-1, 66, 5, 7).float()
        B = x.shape[0]
        x1 = self.first_layer_1d(x[:, :6].permute(0, 3, 1, 2).flatten(2))
        x1 = F.dropout(self.trunk_1d(x1), p=self.dropout, training=self.training)
        pi, v = self.output_layers_PI_1d(x1), self.output_layers_V_1d(x1)
        for m in range(self.N_MACH):
            xm = x[:, 6 + 10 * m:16 + 10 * m].flatten(1)[:, :343].reshape(B, 7, 7, 7).permute(0, 3, 1, 2)
            xm = getattr(self, 'trunk_mach%d' % m)(getattr(self, 'first_layer_mach%d' % m)(xm))
            pi = pi + getattr(self, 'output_layers_PI_mach%d' % m)(xm)
            v = v + getattr(self, 'output_layers_V_mach%d' % m)(xm)
        v = self.final_layers_V(v)
        pi = torch.where(valid_actions.bool(), self.final_layers_PI(pi), self.lowvalue)
        return F.log_softmax(pi, dim=1), torch.tanh(v)


class BotanikV11Module(BotanikV10Module):
    """botanik/BotanikNNet.py nn_version 11 (:162-237, forward :274-289): V10 plus a second machine branch with its own weights
    (first_layer_mach1, trunk_mach1, output_layers_{PI,V}_mach1) on rows 16..25"""
    version = 11
    N_MACH = 2


def loss_pi(target_pi, out_log_pi):                                            # GenericNNetWrapper.py:179-181
    return F.kl_div(out_log_pi, target_pi, reduction='batchmean')


def loss_v(target_z, target_q, out_v, q_weight):                               # :189-191
    t = (target_z + q_weight * target_q) / (1.0 + q_weight)
    return torch.sum((t - out_v) ** 2) / (target_z.shape[0] * target_z.shape[-1])


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sample_ids(n, batch, n_steps, rng_seed, stream0=0, device='cuda:0', out=None):
    """azg_train_sample_ids (include/azg.h; csrc/train.hip.h): np.random.choice(n, batch, replace=False) for n_steps steps in ONE launch
    -> int32[n_steps, batch] on `device`.  Row s is the Fisher-Yates draw of the RNG contract's stream (rng_seed, stream0 + s); nothing is
    synchronised.  out: an int32[n_steps, batch] CUDA tensor to fill instead of a new one."""
    from . import _lib
    if out is None:
        out = torch.empty((max(int(n_steps), 0), max(int(batch), 0)), dtype=torch.int32, device=device)
    assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (n_steps, batch) and out.is_contiguous(), \
        'sample_ids: out must be a contiguous int32[n_steps, batch] CUDA tensor'
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().azg_train_sample_ids(int(n), int(batch), int(n_steps), int(rng_seed) & (2 ** 64 - 1), int(stream0) & (2 ** 64 - 1),
                                                   _ptr(out), _stream()))
    return out


def gather_batch(cols, ids, out=None):
    """azg_train_gather: rows `ids` (int32[B], CUDA) of the five example columns cols = (boards int8[n, S], pi f32[n, A], z f32[n, P], valids
    u8[n, A], q f32[n, P]), contiguous CUDA tensors, in one launch -> (boards int8[B, S], pi, z, valids u8[B, A] holding 0 / 1 -- view it as
    torch.bool --, q).  An id outside [0, n) gives an undefined row.  out: five tensors to fill instead of new ones."""
    from . import _lib
    boards, pi, z, valids, q = cols
    n, S = boards.shape
    A, P, B = pi.shape[1], z.shape[1], ids.shape[0]
    for x, dt, shape in ((boards, torch.int8, (n, S)), (pi, torch.float32, (n, A)), (z, torch.float32, (n, P)), (valids, torch.uint8, (n, A)),
                         (q, torch.float32, (n, P)), (ids, torch.int32, (B,))):
        assert x.is_cuda and x.dtype == dt and tuple(x.shape) == shape and x.is_contiguous() and x.device == boards.device, \
            'gather_batch: dtype / shape / layout of an argument'
    if out is None:
        out = tuple(torch.empty((B, x.shape[1]), dtype=x.dtype, device=x.device) for x in cols)
    for o, x in zip(out, cols):
        assert o.dtype == x.dtype and tuple(o.shape) == (B, x.shape[1]) and o.is_contiguous() and o.device == x.device, \
            'gather_batch: dtype / shape / layout of an output'
    with torch.cuda.device(boards.device):
        _lib.check(_lib.lib().azg_train_gather(_ptr(boards), _ptr(pi), _ptr(z), _ptr(valids), _ptr(q), _ptr(ids), n, B, S, A, P,
                                               *[_ptr(o) for o in out], _stream()))
    return tuple(out)


def gather_forms(game_id, variant, records, first_row, row_end, streams, ids, rng_seed, out=None):
    """azg_train_gather_forms: the batch rows `ids` (int32[B], CUDA) of the VIRTUAL rows that the n records = (boards int8[n, S], pi
    f32[n, A], z f32[n, P], valids u8[n, A], q f32[n, P]) expand to -- form k of record g is virtual row first_row[g] + k, its live rows end
    at row_end[g] (int64[n], non-decreasing), its forms draw from stream (rng_seed, streams[g]) (int64 / uint64 bits [n], or None = g) --
    computed in one launch, without the expanded rows ever being stored (history.CompactHistory.gather) -> the five batch tensors of
    gather_batch.  An id that no record owns gives an undefined row.  out: five tensors to fill instead of new ones."""
    from . import _lib
    boards, pi, z, valids, q = records
    n, S = boards.shape
    A, P, B = pi.shape[1], z.shape[1], ids.shape[0]
    for x, dt, shape in ((boards, torch.int8, (n, S)), (pi, torch.float32, (n, A)), (z, torch.float32, (n, P)), (valids, torch.uint8, (n, A)),
                         (q, torch.float32, (n, P)), (first_row, torch.int64, (n,)), (row_end, torch.int64, (n,)), (ids, torch.int32, (B,))):
        assert x.is_cuda and x.dtype == dt and tuple(x.shape) == shape and x.is_contiguous() and x.device == boards.device, \
            'gather_forms: dtype / shape / layout of an argument'
    assert streams is None or (streams.is_cuda and streams.dtype in (torch.int64, torch.uint64) and tuple(streams.shape) == (n,) and
                               streams.is_contiguous() and streams.device == boards.device), 'gather_forms: streams'
    if out is None:
        out = tuple(torch.empty((B, x.shape[1]), dtype=x.dtype, device=x.device) for x in records)
    for o, x in zip(out, records):
        assert o.dtype == x.dtype and tuple(o.shape) == (B, x.shape[1]) and o.is_contiguous() and o.device == x.device, \
            'gather_forms: dtype / shape / layout of an output'
    with torch.cuda.device(boards.device):
        _lib.check(_lib.lib().azg_train_gather_forms(int(game_id), int(variant), _ptr(boards), _ptr(pi), _ptr(z), _ptr(valids), _ptr(q),
                                                     _ptr(first_row), _ptr(row_end), None if streams is None else _ptr(streams), n, _ptr(ids), B,
                                                     *[_ptr(o) for o in out], int(rng_seed) & (2 ** 64 - 1), _stream()))
    return tuple(out)


def train_losses(log_pi, v, target_pi, z, q, q_weight, v_coeff=0.25, out=None):
    """azg_train_losses on contiguous f32 CUDA tensors (log_pi / target_pi [B, A], v / z / q [B, P]) -> (grad_log_pi f32[B, A], grad_v
    f32[B, P], rows f64[B, 2], out f64[2]): the row sums and the totals (loss_pi, loss_v) of include/azg.h, and the gradient of loss_pi +
    v_coeff * loss_v with respect to log_pi and v.  The buffers are allocated here (out too when None): the C call owns no memory.  Two
    launches on the current stream, nothing synchronised."""
    from . import _lib
    B, A = log_pi.shape
    P = v.shape[1]
    for x, shape in ((log_pi, (B, A)), (target_pi, (B, A)), (v, (B, P)), (z, (B, P)), (q, (B, P))):
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == shape and x.is_contiguous() and x.device == log_pi.device, \
            'train_losses: dtype / shape / layout of an argument'
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=log_pi.device)
    assert out.dtype == torch.float64 and tuple(out.shape) == (2,) and out.is_contiguous() and out.device == log_pi.device, \
        'train_losses: out must be a contiguous f64[2] tensor on the same device'
    g_pi, g_v = torch.empty_like(log_pi), torch.empty_like(v)
    rows = torch.empty((B, 2), dtype=torch.float64, device=log_pi.device)
    with torch.cuda.device(log_pi.device):
        _lib.check(_lib.lib().azg_train_losses(_ptr(log_pi), _ptr(v), _ptr(target_pi), _ptr(z), _ptr(q), B, A, P, C.c_float(float(q_weight)),
                                               C.c_float(float(v_coeff)), _ptr(g_pi), _ptr(g_v), _ptr(rows), _ptr(out), _stream()))
    return g_pi, g_v, rows, out


class _FusedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_pi, v, target_pi, z, q, q_weight, v_coeff, out):
        g_pi, g_v, _, out = train_losses(log_pi.contiguous(), v.contiguous(), target_pi, z, q, q_weight, v_coeff, out)
        ctx.save_for_backward(g_pi, g_v)
        return (out[0] + float(v_coeff) * out[1]).to(torch.float32)

    @staticmethod
    def backward(ctx, grad_output):
        g_pi, g_v = ctx.saved_tensors
        return g_pi * grad_output, g_v * grad_output, None, None, None, None, None, None


def fused_loss(log_pi, v, target_pi, z, q, q_weight, v_coeff=0.25, out=None):
    """L = loss_pi(target_pi, log_pi) + v_coeff * loss_v(z, q, v, q_weight) as an f32 scalar with its backward pass, by azg_train_losses
    (include/azg.h; csrc/train.hip.h): two launches forward, which also write the gradients with respect to log_pi and v; backward hands
    them on, scaled by grad_output on the device.  log_pi f32[B, A] LOG-probabilities, v f32[B, P] (the module's outputs), target_pi
    f32[B, A], z / q f32[B, P], all CUDA.  out: an f64[2] tensor that receives (loss_pi, loss_v) -- e.g. a row of a per-epoch buffer, read
    once; a new one when None.  Nothing is synchronised."""
    return _FusedLoss.apply(log_pi, v, target_pi, z, q, q_weight, v_coeff, out)


def onecycle_adamw_table(max_lr, total_steps, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
    """-> numpy f32[total_steps, 8]: row s holds the scalars torch.optim.AdamW uses in optimiser step s (0-based) when
    OneCycleLR(opt, max_lr=max_lr, total_steps=total_steps) has been stepped s times after construction (the table of azg_train_adamw,
    include/azg.h):  { 1 - lr wd, 1 - beta1, beta2, 1 - beta2, lr / (1 - beta1^k), (1 - beta2^k)^0.5, eps, 0 },  k = s + 1.
    lr and beta1 (OneCycleLR cycles the momentum, 0.95 -> 0.85 -> 0.95) are read from torch's own scheduler, run here once on a dummy
    one-parameter AdamW; the rest is derived in Python floats exactly as torch's _multi_tensor_adamw does (the bias correction with the
    CURRENT beta1), and every value is cast to f32 once."""
    total_steps = int(total_steps)
    if total_steps < 1:
        raise ValueError('onecycle_adamw_table: total_steps >= 1 is required, got %d' % total_steps)
    opt = torch.optim.AdamW([nn.Parameter(torch.zeros(1))], lr=max_lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=max_lr, total_steps=total_steps)
    table = np.zeros((total_steps, 8), dtype=np.float32)
    for s in range(total_steps):
        group = opt.param_groups[0]
        lr, (beta1, beta2), k = float(group['lr']), (float(b) for b in group['betas']), float(s + 1)
        table[s] = [1 - lr * weight_decay, 1 - beta1, beta2, 1 - beta2, lr / (1 - beta1 ** k), (1 - beta2 ** k) ** 0.5, eps, 0.0]
        if s + 1 < total_steps:
            opt.step()                                                       # (no gradient: a no-op that keeps the scheduler's call order)
            sched.step()
    return table


ADAMW_CHUNK = 2048                                                           # csrc/train.hip.h TRAIN_ADAMW_CHUNK


def adamw_tables(quads):
    """The segment and chunk tables of azg_train_adamw for quads = [(p, g, m, v), ...], contiguous f32 CUDA tensors of one numel per
    quadruple (any alignment, any offset into their storage) -> (segs int64[n, 5], chunks int32[n_chunks, 2]) on the tensors' device.
    The tables hold the tensors' addresses: they are good for as long as the tensors are."""
    segs, chunks, dev = [], [], None
    for k, quad in enumerate(quads):
        n = quad[0].numel()
        dev = quad[0].device if dev is None else dev
        for t in quad:
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n and t.device == dev):
                raise ValueError('adamw_tables: p, g, m and v of a segment must be contiguous f32 CUDA tensors of one size on one device')
        if n >= 2 ** 31:
            raise ValueError('adamw_tables: a segment must hold fewer than 2^31 elements')
        segs.append([t.data_ptr() for t in quad] + [n])
        chunks.extend((k, first) for first in range(0, n, ADAMW_CHUNK))
    if not chunks:
        raise ValueError('adamw_tables: no element to update')
    return (torch.tensor(segs, dtype=torch.int64).to(dev), torch.tensor(chunks, dtype=torch.int32).to(dev))


def adamw_update(segs, chunks, table, step):
    """azg_train_adamw: one launch on the current stream updates every segment of adamw_tables() with row clamp(step[0], 0, len(table) - 1)
    of table (f32[total_steps, 8], CUDA); step is an int64[1] CUDA tensor that the launch only reads.  Nothing is synchronised."""
    from . import _lib
    assert segs.is_cuda and segs.dtype == torch.int64 and segs.dim() == 2 and segs.shape[1] == 5 and segs.is_contiguous(), 'adamw_update: segs'
    assert chunks.dtype == torch.int32 and chunks.dim() == 2 and chunks.shape[1] == 2 and chunks.is_contiguous(), 'adamw_update: chunks'
    assert table.dtype == torch.float32 and table.dim() == 2 and table.shape[1] == 8 and table.is_contiguous(), 'adamw_update: table'
    assert step.dtype == torch.int64 and step.numel() == 1, 'adamw_update: step'
    assert chunks.device == segs.device and table.device == segs.device and step.device == segs.device, 'adamw_update: one device'
    with torch.cuda.device(segs.device):
        _lib.check(_lib.lib().azg_train_adamw(_ptr(segs), segs.shape[0], _ptr(chunks), chunks.shape[0], _ptr(table), table.shape[0], _ptr(step),
                                              _stream()))


def adamw_step_advance(step):
    """azg_train_step_advance: step[0] += 1 (int64[1], CUDA) in a launch of its own on the current stream"""
    from . import _lib
    assert step.is_cuda and step.dtype == torch.int64 and step.numel() == 1, 'adamw_step_advance: step must be an int64[1] CUDA tensor'
    with torch.cuda.device(step.device):
        _lib.check(_lib.lib().azg_train_step_advance(_ptr(step), _stream()))


class DeviceAdamW:
    """torch.optim.AdamW(params, lr=max_lr, betas, eps, weight_decay) under OneCycleLR(max_lr=max_lr, total_steps=total_steps) with no
    per-step value on the host: step() is azg_train_adamw + azg_train_step_advance (csrc/train.hip.h) on the current stream, the step number
    lives in device memory (step_counter, never read back) and picks a row of onecycle_adamw_table.  No amsgrad, no maximize.
    It owns one flat f32 buffer each for the moments m and v (zeroed) and one for the gradients; a parameter's segment starts at a multiple
    of 4 floats.  The parameters must be contiguous f32 CUDA tensors that stay where they are (call module.to(device) first).
    The FIRST backward runs with every .grad unset: step() then knows which parameters received a gradient -- one that requires grad and
    got none raises ValueError (torch would skip it; one launch over fixed tables cannot) -- moves the gradients into the flat buffer and
    makes every .grad a view of it.  From then on zero_grad() is one memset and backward accumulates into the views (0 + g is g)."""

    def __init__(self, params, max_lr, total_steps, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        self.params = [p for p in params if p.requires_grad and p.numel() > 0]
        if not self.params:
            raise ValueError('DeviceAdamW: no parameter to optimise')
        dev = self.params[0].device
        for p in self.params:
            if not (p.is_cuda and p.device == dev and p.dtype == torch.float32 and p.is_contiguous()):
                raise ValueError('DeviceAdamW: the parameters must be contiguous f32 CUDA tensors on one device')
        self.total_steps = int(total_steps)
        self.offsets, total = [], 0
        for p in self.params:
            self.offsets.append(total)
            total += -(-p.numel() // 4) * 4
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.table = torch.from_numpy(onecycle_adamw_table(max_lr, self.total_steps, betas, eps, weight_decay)).to(dev)
        self.step_counter = torch.zeros(1, dtype=torch.int64, device=dev)
        cut = lambda flat: [flat[o:o + p.numel()] for o, p in zip(self.offsets, self.params)]  # noqa: E731
        self.grad_views = [g.view_as(p) for g, p in zip(cut(self.flat_grad), self.params)]
        self.segs, self.chunks = adamw_tables(list(zip([p.detach() for p in self.params], cut(self.flat_grad), cut(self.exp_avg),
                                                       cut(self.exp_avg_sq))))
        self.steps_taken = 0                                                   # the host's count: the device counter is never read back
        self._adopted = False
        for p in self.params:
            p.grad = None

    def zero_grad(self):
        if self._adopted:
            self.flat_grad.zero_()

    def _check_limit(self):
        if self.steps_taken >= self.total_steps:
            raise ValueError('DeviceAdamW: tried to step %d times, the schedule has total_steps = %d' % (self.steps_taken + 1, self.total_steps))

    def count_step(self):
        """the host's count of one step; raises before a (total_steps + 1)-th, where OneCycleLR raises"""
        self._check_limit()
        self.steps_taken += 1

    def launch(self):
        """the two launches of a step without the host's count -- what a graph captures (count_step() then goes with each replay)"""
        if not self._adopted:
            missing = [k for k, p in enumerate(self.params) if p.grad is None]
            if missing:
                raise ValueError('DeviceAdamW: %d of %d parameters that require grad received none in the first backward (the first is '
                                 'number %d, shape %s): freeze it (requires_grad=False) or leave it out' %
                                 (len(missing), len(self.params), missing[0], tuple(self.params[missing[0]].shape)))
            torch._foreach_copy_(self.grad_views, [p.grad for p in self.params])
            for p, g in zip(self.params, self.grad_views):
                p.grad = g
            self._adopted = True
        adamw_update(self.segs, self.chunks, self.table, self.step_counter)
        adamw_step_advance(self.step_counter)

    def step(self):
        self._check_limit()
        self.launch()
        self.steps_taken += 1


def train(module, examples, learn_rate=3e-3, batch_size=512, epochs=2, q_weight=0.5, device='cuda:0', seed=None, log=None, board_shape=None,
          device_batches=False, batch_ids=None, device_optimizer=False, graph_step=False, info=None, on_step=None):
    """examples = (boards int8[n,S], pi f32[n,A], z f32[n,P], valids u8/bool[n,A], q f32[n,P]) tensors or arrays -- or, with
    device_batches=True, a history.CompactHistory: n is then its number of virtual rows and every batch is computed from its records
    (azg_train_gather_forms); sampling, batch_ids, losses, optimiser and graph capture are the same.
    board_shape: give it for a module that expects the reference's inputs (float boards of getBoardSize(), bool valids:
    GenericNNetWrapper.py:60-63) instead of the engine modules' flat int8 boards.
    on_step(epoch, i_batch, step): called after every optimiser + scheduler step (step = i_batch + steps_per_epoch * epoch) -- the hook of
    the reference's periodic validation (:86-90); it must leave the module in train() mode.  With None nothing changes, random stream included.
    batch_ids: an int array [epochs * steps_per_epoch, batch_size]: row `step` is that step's batch instead of a draw (either path; the
    generator is then not used).
    device_batches=True (CUDA only): the batches never touch the host -- _train_device_batches.  With the defaults nothing changes.
    device_optimizer=True (needs device_batches=True and a CUDA device): DeviceAdamW in place of torch's AdamW + OneCycleLR -- the update of
    all parameters and the schedule in one launch (azg_train_adamw), the step number in device memory.  Still eager, the same call order.
    graph_step=True (implies device_optimizer=True): step 0 runs eagerly on a side stream -- the warm-up that a capture needs, and a real
    training step --, then ONE step (row pick, gather, forward, loss, backward, optimiser) is captured with torch.cuda.graph and every later
    step is one replay.  on_step is still called from the host after every step, on weights that are updated in place.  A module that cannot
    be captured raises: there is no fallback.  With a single step in all nothing is captured.  Under capture dropout draws from torch's
    graph-safe Philox state: with dropout > 0 its random stream differs from the eager paths'.
    info: a dict that receives {'optimizer': 'torch' | 'device', 'graph_replays': int}.
    Returns the list of (pi loss, v loss) per step."""
    device_optimizer = bool(device_optimizer) or bool(graph_step)
    if device_optimizer and torch.device(device).type != 'cuda':
        raise ValueError('train: device_optimizer=True%s needs a CUDA device, got %r (there is no CPU form of the optimiser kernel)'
                         % (' (implied by graph_step=True)' if graph_step else '', device))
    if device_optimizer and not device_batches:
        raise ValueError('train: device_optimizer=True%s needs device_batches=True' % (' (implied by graph_step=True)' if graph_step else ''))
    if isinstance(info, dict):
        info.update(optimizer='device' if device_optimizer else 'torch', graph_replays=0)
    if device_batches:
        return _train_device_batches(module, examples, learn_rate, batch_size, epochs, q_weight, device, seed, log, board_shape, on_step, batch_ids,
                                     device_optimizer, bool(graph_step), info if isinstance(info, dict) else None)
    if _is_compact(examples):
        raise ValueError('train: a CompactHistory holds records, not rows; only device_batches=True reads it (its gather computes the rows of '
                         'a batch on the GPU)')
    boards, pi, z, valids, q = [torch.as_tensor(np.asarray(x.cpu()) if hasattr(x, 'cpu') else x).to(device) for x in examples[:5]]
    n = boards.shape[0]
    valids = valids.bool()
    if board_shape is not None:
        boards = boards.reshape((n,) + tuple(board_shape)).to(torch.float32)
    steps_per_epoch = n // batch_size
    if steps_per_epoch == 0:
        raise ValueError('fewer examples (%d) than batch_size (%d)' % (n, batch_size))
    if batch_ids is not None:
        batch_ids = _check_batch_ids(batch_ids, epochs * steps_per_epoch, batch_size).to(device)
    module.to(device).train()
    opt = torch.optim.AdamW(module.parameters(), lr=learn_rate)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=learn_rate, steps_per_epoch=steps_per_epoch, epochs=epochs)
    gen = torch.Generator(device='cpu')
    if seed is not None:
        gen.manual_seed(seed)
    hist = []
    for ep in range(epochs):
        for i_batch in range(steps_per_epoch):
            if batch_ids is not None:
                ids = batch_ids[i_batch + steps_per_epoch * ep]
            else:
                ids = torch.randperm(n, generator=gen)[:batch_size].to(device)   # np.random.choice(n, batch, replace=False) :57
            opt.zero_grad(set_to_none=True)
            out_pi, out_v = module(boards[ids], valids[ids])
            l_pi = loss_pi(pi[ids].float(), out_pi)
            l_v = loss_v(z[ids].float(), q[ids].float(), out_v, q_weight)
            (l_pi + 0.25 * l_v).backward()
            opt.step()
            sched.step()
            hist.append((l_pi.item(), l_v.item()))
            if on_step is not None:
                on_step(ep, i_batch, i_batch + steps_per_epoch * ep)
        if log:
            log('epoch %d: pi loss %.4f  v loss %.4f' % (ep + 1, np.mean([h[0] for h in hist[-steps_per_epoch:]]),
                                                         np.mean([h[1] for h in hist[-steps_per_epoch:]])))
    module.eval()
    return hist


def _is_compact(examples):
    from .history import CompactHistory
    return isinstance(examples, CompactHistory)


def _check_batch_ids(batch_ids, steps, batch_size):
    """-> int64 CPU tensor [steps, batch_size]"""
    ids = torch.as_tensor(np.asarray(batch_ids.cpu()) if hasattr(batch_ids, 'cpu') else np.asarray(batch_ids))
    if ids.dtype.is_floating_point or ids.dtype == torch.bool or tuple(ids.shape) != (steps, batch_size):
        raise ValueError('batch_ids must be an int array [epochs * steps_per_epoch, batch_size] = [%d, %d], got %s %s'
                         % (steps, batch_size, ids.dtype, tuple(ids.shape)))
    return ids.long()


def _train_device_batches(module, examples, learn_rate, batch_size, epochs, q_weight, device, seed, log, board_shape, on_step, batch_ids,
                          device_optimizer=False, graph_step=False, info=None):
    """train() with the batches drawn, gathered and scored on the GPU (csrc/train.hip.h): the columns are made contiguous on the device once;
    one sample_ids launch draws an epoch's ids (rng_seed = seed, or fresh entropy when None; stream0 = epoch * steps_per_epoch); a step is
    gather_batch, the module's forward, fused_loss, backward, opt.step(), sched.step(); the losses land in a device buffer f64[steps, 2]
    that is read once per epoch.  The host waits for the GPU at the end of an epoch only (and wherever on_step does).
    device_optimizer: DeviceAdamW is both opt and sched.  graph_step: _train_graph_steps runs the steps."""
    if torch.device(device).type != 'cuda':
        raise ValueError('train: device_batches=True needs a CUDA device, got %r (there is no CPU form of the batch kernels)' % (device,))
    dev = torch.device(device)
    if _is_compact(examples):                                                # the records stay what they are: n counts the VIRTUAL rows and
        if examples.device != dev:                                           # history.gather computes the rows a batch names
            raise ValueError('train: the CompactHistory lives on %s, the training runs on %s' % (examples.device, dev))
        cols, n = examples, int(examples.n)
        gather = examples.gather
    else:
        boards, pi, z, valids, q = [x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x)) for x in examples[:5]]
        n = int(boards.shape[0])
        cols = (boards.to(dev).reshape(n, -1).to(torch.int8).contiguous(), pi.to(dev).reshape(n, -1).to(torch.float32).contiguous(),
                z.to(dev).reshape(n, -1).to(torch.float32).contiguous(), (valids.to(dev).reshape(n, -1) != 0).view(torch.uint8).contiguous(),
                q.to(dev).reshape(n, -1).to(torch.float32).contiguous())
        gather = lambda ids, out=None: gather_batch(cols, ids, out=out)      # noqa: E731
    steps_per_epoch = n // batch_size
    if steps_per_epoch == 0:
        raise ValueError('fewer examples (%d) than batch_size (%d)' % (n, batch_size))
    if batch_ids is not None:
        ids_all = _check_batch_ids(batch_ids, epochs * steps_per_epoch, batch_size)
        if ids_all.numel() and (int(ids_all.min()) < 0 or int(ids_all.max()) >= n):
            raise ValueError('batch_ids holds an id outside [0, %d)' % n)
        ids_all = ids_all.to(torch.int32).to(dev)
    else:
        rng_seed = int.from_bytes(os.urandom(8), 'little') if seed is None else int(seed)
    module.to(dev).train()
    if device_optimizer:
        opt, sched = DeviceAdamW(module.parameters(), learn_rate, epochs * steps_per_epoch), None
    else:
        opt = torch.optim.AdamW(module.parameters(), lr=learn_rate)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=learn_rate, steps_per_epoch=steps_per_epoch, epochs=epochs)
    hist = []
    with torch.cuda.device(dev):
        if graph_step:
            if batch_ids is None:                                            # every epoch's ids before the capture: row s of epoch e is
                ids_all = sample_ids(n, batch_size, epochs * steps_per_epoch, rng_seed, 0, device=dev)   # stream e * steps_per_epoch + s
            hist = _train_graph_steps(module, cols, ids_all, opt, batch_size, epochs, steps_per_epoch, q_weight, board_shape, on_step, log, info,
                                      gather)
            module.eval()
            return hist
        for ep in range(epochs):
            if batch_ids is not None:
                ids_ep = ids_all[ep * steps_per_epoch:(ep + 1) * steps_per_epoch]
            else:
                ids_ep = sample_ids(n, batch_size, steps_per_epoch, rng_seed, ep * steps_per_epoch, device=dev)
            losses = torch.empty((steps_per_epoch, 2), dtype=torch.float64, device=dev)
            for i_batch in range(steps_per_epoch):
                b_boards, b_pi, b_z, b_valids, b_q = gather(ids_ep[i_batch])
                if board_shape is not None:
                    b_boards = b_boards.reshape((batch_size,) + tuple(board_shape)).to(torch.float32)
                if sched is None:
                    opt.zero_grad()
                else:
                    opt.zero_grad(set_to_none=True)
                out_pi, out_v = module(b_boards, b_valids.view(torch.bool))
                fused_loss(out_pi, out_v, b_pi, b_z, b_q, q_weight, 0.25, out=losses[i_batch]).backward()
                opt.step()
                if sched is not None:
                    sched.step()
                if on_step is not None:
                    on_step(ep, i_batch, i_batch + steps_per_epoch * ep)
            got = losses.cpu().numpy()                                       # the epoch's one read
            hist.extend((float(a), float(b)) for a, b in got)
            if log:
                log('epoch %d: pi loss %.4f  v loss %.4f' % (ep + 1, got[:, 0].mean(), got[:, 1].mean()))
    module.eval()
    return hist


def _train_graph_steps(module, cols, ids_all, opt, batch_size, epochs, steps_per_epoch, q_weight, board_shape, on_step, log, info, gather=None):
    """The steps of train(graph_step=True), the current device being the columns': ids_all int32[total_steps, batch] on the device, opt a
    DeviceAdamW.  cols: the five columns, or a CompactHistory with gather = its gather (the batch rows are then computed, not copied).  The step body reads no host value that changes: its row of ids_all and its row of the loss buffer are picked by a device
    index made from opt.step_counter with torch ops, and the optimiser takes its scalars by the same counter.  Everything is enqueued on
    one stream, so the captured graph is one linear chain."""
    if gather is None:
        gather = lambda ids, out=None: gather_batch(cols, ids, out=out)      # noqa: E731
    rec = cols.record_columns() if _is_compact(cols) else cols               # (the widths and dtypes of a batch are the records')
    dev = rec[0].device
    total = epochs * steps_per_epoch
    losses = torch.zeros((total, 2), dtype=torch.float64, device=dev)
    loss2 = torch.zeros(2, dtype=torch.float64, device=dev)
    outs = tuple(torch.empty((batch_size, x.shape[1]), dtype=x.dtype, device=dev) for x in rec)

    def body():
        idx = opt.step_counter.clamp(0, total - 1)                           # int64[1]: this step's number
        gather(ids_all.index_select(0, idx)[0], out=outs)
        b_boards = outs[0]
        if board_shape is not None:
            b_boards = b_boards.reshape((batch_size,) + tuple(board_shape)).to(torch.float32)
        opt.zero_grad()
        out_pi, out_v = module(b_boards, outs[3].view(torch.bool))
        loss = fused_loss(out_pi, out_v, outs[1], outs[2], outs[4], q_weight, 0.25, out=loss2)
        losses.index_copy_(0, idx, loss2[None])
        loss.backward()
        opt.launch()

    side = torch.cuda.Stream(device=dev)                                     # step 0, eagerly: the warm-up of torch's capture recipe
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.count_step()
        body()
    torch.cuda.current_stream().wait_stream(side)
    graph, hist = None, []
    for ep in range(epochs):
        for i_batch in range(steps_per_epoch):
            step = i_batch + steps_per_epoch * ep
            if step > 0:
                if graph is None:
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        body()
                opt.count_step()
                graph.replay()
                if info is not None:
                    info['graph_replays'] += 1
            if on_step is not None:
                on_step(ep, i_batch, step)
        got = losses[ep * steps_per_epoch:(ep + 1) * steps_per_epoch].cpu().numpy()     # the epoch's one read
        hist.extend((float(a), float(b)) for a, b in got)
        if log:
            log('epoch %d: pi loss %.4f  v loss %.4f' % (ep + 1, got[:, 0].mean(), got[:, 1].mean()))
    return hist
