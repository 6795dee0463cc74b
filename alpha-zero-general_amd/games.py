"""Game.py-compatible env plugins backed by the batched HIP env kernels (azg_env_* in include/azg.h).

Same method names, argument meaning and return types as the reference's adaptors (splendor/SplendorGame.py:16-60,
santorini/SantoriniGame.py:16-60, Game.py:14-162).  Every method also has a `*_batch` twin that takes and returns
torch CUDA tensors for n boards at once -- that is the form the engine itself uses."""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, lib


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


Playouts = collections.namedtuple('Playouts', 'ended plies status boards players actions')


def playouts_into(game, boards, players, k, max_plies, active, stream0, counters, ended, plies, status, out_boards=None, out_players=None,
                  out_actions=None):
    """azg_env_playouts (include/azg.h) into tensors the caller owns: k random playouts from each of boards int8[n, S] (players int32[n] or
    None, active u8 / bool[n] or None, counters int64[n * k] or None) -> ended f32[n, k, P], plies int32[n, k], status u8[n, k] and, where
    given, out_boards int8[n, k, S], out_players int32[n, k], out_actions int32[n, k, max_plies].  Rows of a board with active == 0 are
    left as they are.  One launch on the current stream, nothing allocated, nothing synchronised."""
    n, k, max_plies = boards.shape[0], int(k), int(max_plies)
    boards = boards.reshape(n, -1)
    assert boards.dtype == torch.int8 and boards.is_contiguous() and boards.shape[1] == game.S
    for x, dt, shape in ((players, (torch.int32,), (n,)), (active, (torch.uint8, torch.bool), (n,)), (counters, (torch.int64,), (n * k,)),
                         (ended, (torch.float32,), (n, k, game.P)), (plies, (torch.int32,), (n, k)), (status, (torch.uint8,), (n, k)),
                         (out_boards, (torch.int8,), (n, k, game.S)), (out_players, (torch.int32,), (n, k)),
                         (out_actions, (torch.int32,), (n, k, max_plies))):
        assert x is None or (x.dtype in dt and tuple(x.shape) == shape and x.is_contiguous() and x.device == boards.device), \
            'playouts: dtype / shape / layout of an argument'
    check(lib().azg_env_playouts(game.GAME_ID, game.variant, _ptr(boards), _ptr(players), _ptr(active), n, k, max_plies,
                                 C.c_uint64(int(game.rng_seed) & (2 ** 64 - 1)), C.c_uint64(int(stream0) & (2 ** 64 - 1)), _ptr(counters),
                                 _ptr(ended), _ptr(plies), _ptr(status), _ptr(out_boards), _ptr(out_players), _ptr(out_actions), _stream()))


Lookahead = collections.namedtuple('Lookahead', 'valid scores ended next_player states')
INT32_MIN = -2 ** 31
GREEDY_RULES = {'reference': 0, 'lead': 1}                   # AZG_GREEDY_REFERENCE, AZG_GREEDY_LEAD (include/azg.h)


def default_waves_per_state(A):
    """waves of azg_env_lookahead per position when the caller names none.  Every wave of a position re-reads the state and rebuilds the
    whole valid mask -- work that grows with A -- before it steps its share of the valid moves, so the rule follows A:
        A <= 256          min(8, ceil(A / 8)): a wave per 8 ids, 8 for Splendor (81) and Santorini without gods (162), where the mask is
                          cheap next to 35-49 steps per position -- within 3 % of the best of the sweep at 4096 positions, 4-7 times
                          faster than one wave at 64;
        256 < A <= 1024   4 (not measured: between the two);
        A > 1024          2: every further wave re-does Abalone's mask over 3402 ids, which at 4096 positions costs more than sharing the
                          64 steps saves -- one wave is best there and two cost 6 % more; at 64 positions two take 30 % less than one.
    The sweep is in profiles/r17_lookahead.md.  The result never depends on the number."""
    A = int(A)
    return max(1, min(8, (A + 7) // 8)) if A <= 256 else 4 if A <= 1024 else 2


def greedy_candidates(game, rule, canonical, valid, scores, active=None, out=None):
    """azg_greedy_candidates (include/azg.h): the greedy players' candidate sets u8[n, A] for canonical boards int8[n, S] from what
    lookahead_batch gave for them (valid u8[n, A], scores int32[n, A, P]; scores may be None for Azul's reference rule).  rule:
    'reference' (the reference's GreedyPlayer: Splendor, Azul, Abalone) or 'lead' (the mover's lead after the move: any game).  Rows with
    active == 0 keep what `out` (zeros when not given) holds."""
    n = canonical.shape[0]
    canonical = canonical.reshape(n, game.S)
    if out is None:
        out = torch.zeros((n, game.A), dtype=torch.uint8, device=canonical.device)
    for x, dt, shape in ((canonical, (torch.int8,), (n, game.S)), (valid, (torch.uint8,), (n, game.A)), (scores, (torch.int32,), (n, game.A, game.P)),
                         (active, (torch.uint8, torch.bool), (n,)), (out, (torch.uint8,), (n, game.A))):
        assert x is None or (x.dtype in dt and tuple(x.shape) == shape and x.is_contiguous() and x.device == canonical.device), \
            'greedy_candidates: dtype / shape / layout of an argument'
    check(lib().azg_greedy_candidates(game.GAME_ID, game.variant, GREEDY_RULES[rule], _ptr(canonical), _ptr(valid), _ptr(scores), n, _ptr(active),
                                      _ptr(out), _stream()))
    return out


class HipGame:
    GAME_ID = None

    def __init__(self, variant, device='cuda:0', rng_seed=0):
        if not torch.cuda.is_available():
            raise _lib.AzgError('no GPU visible: the engine has no CPU fallback')
        self.variant = variant
        self.device = torch.device(device)
        self.S, self.A, self.P, self.rows, self.cols = _lib.game_info(self.GAME_ID, variant)
        self.num_players = self.P
        self.rng_seed = rng_seed
        self._stream_ctr = 0
        self._draw = torch.zeros(1, dtype=torch.int64, device=self.device)

    # ---- batch API (torch CUDA tensors) ----
    def valid_moves_batch(self, boards, players):
        n = boards.shape[0]
        out = torch.empty((n, self.A), dtype=torch.uint8, device=self.device)
        check(lib().azg_env_valid_moves(self.GAME_ID, self.variant, _ptr(boards), _ptr(players), n, _ptr(out),
                                        _stream()))
        return out

    def next_state_batch(self, boards, players, actions, seeds, stream0=0, counters=None):
        n = boards.shape[0]
        out = torch.empty((n, self.S), dtype=torch.int8, device=self.device)
        nxt = torch.empty((n,), dtype=torch.int32, device=self.device)
        check(lib().azg_env_next_state(self.GAME_ID, self.variant, _ptr(boards), _ptr(players), _ptr(actions),
                                       _ptr(seeds), n, _ptr(out), _ptr(nxt), self.rng_seed, stream0, _ptr(counters),
                                       _stream()))
        return out, nxt

    def game_ended_batch(self, boards, next_players):
        n = boards.shape[0]
        ended = torch.empty((n, self.P), dtype=torch.float32, device=self.device)
        scores = torch.empty((n, self.P), dtype=torch.int32, device=self.device)
        rnd = torch.empty((n,), dtype=torch.int32, device=self.device)
        check(lib().azg_env_game_ended(self.GAME_ID, self.variant, _ptr(boards), _ptr(next_players), n, _ptr(ended),
                                       _ptr(scores), _ptr(rnd), _stream()))
        return ended, scores, rnd

    def canonical_batch(self, boards, players):
        n = boards.shape[0]
        out = torch.empty((n, self.S), dtype=torch.int8, device=self.device)
        check(lib().azg_env_canonical(self.GAME_ID, self.variant, _ptr(boards), _ptr(players), n, _ptr(out), _stream()))
        return out

    def init_boards_batch(self, n, stream0=0, counters=None):
        """Board.init_game for n games on RNG streams stream0..stream0+n-1; `counters` (u64[n] tensor) receives the number
        of uniforms each stream consumed, so next_state_batch(..., counters=counters) continues the same streams"""
        out = torch.empty((n, self.S), dtype=torch.int8, device=self.device)
        check(lib().azg_env_init_boards(self.GAME_ID, self.variant, n, _ptr(out), self.rng_seed, stream0, _ptr(counters),
                                        _stream()))
        return out

    def playouts_batch(self, boards, players=None, k=1, max_plies=4096, active=None, stream0=0, counters=None, final_boards=False,
                       trace=False):
        """k random playouts from each of n boards, each to the end of its game, in one launch (azg_env_playouts): every move uniform among
        the valid ones, playout j of board t on RNG stream stream0 + t * k + j from counters[t * k + j] (int64[n * k], advanced in place;
        None: from 0).  -> Playouts(ended f32[n, k, P] in the seat numbering of the input board, plies i32[n, k], status u8[n, k]: 0
        finished / 1 max_plies reached / 2 no valid move (ended is zero for 1 and 2), boards int8[n, k, S] and players i32[n, k] at the end
        with final_boards, actions i32[n, k, max_plies] (-1 past plies) with trace).  Rows of a board with active == 0 come back as zeros
        (actions -1) and keep their counters."""
        n, dev = boards.shape[0], self.device
        ended = torch.zeros((n, k, self.P), dtype=torch.float32, device=dev)
        plies = torch.zeros((n, k), dtype=torch.int32, device=dev)
        status = torch.zeros((n, k), dtype=torch.uint8, device=dev)
        ob = torch.zeros((n, k, self.S), dtype=torch.int8, device=dev) if final_boards else None
        op = torch.zeros((n, k), dtype=torch.int32, device=dev) if final_boards else None
        oa = torch.full((n, k, max_plies), -1, dtype=torch.int32, device=dev) if trace else None
        playouts_into(self, boards, players, k, max_plies, active, stream0, counters, ended, plies, status, ob, op, oa)
        return Playouts(ended, plies, status, ob, op, oa)

    def lookahead_batch(self, boards, players=None, active=None, waves_per_state=None, stream0=0, counters=None, successor_states=False):
        """all successors of n boards in one launch (azg_env_lookahead): for every valid action a of board t, what next_state_batch
        (random_seed 0, stream stream0 + t, from counters[t]: int64[n], never written; None: from 0) and game_ended_batch give for it.
        -> Lookahead(valid u8[n, A], scores i32[n, A, P], ended f32[n, A, P], next_player i32[n, A], states int8[n, A, S] with
        successor_states else None), in the seat numbering of the input boards.  Rows of invalid actions, and every row of a board with
        active == 0 (valid included), hold the fill values: scores INT32_MIN, ended 0, next_player -1, states 0, valid 0.
        waves_per_state (1 .. 64; None: default_waves_per_state(A)) only deals the work out, the result does not depend on it."""
        n, dev = boards.shape[0], self.device
        boards = boards.reshape(n, self.S)
        assert boards.dtype == torch.int8 and boards.is_contiguous()
        for x, dt in ((players, (torch.int32,)), (active, (torch.uint8, torch.bool)), (counters, (torch.int64,))):
            assert x is None or (x.dtype in dt and tuple(x.shape) == (n,) and x.is_contiguous() and x.device == boards.device), \
                'lookahead: dtype / shape / layout of an argument'
        W = default_waves_per_state(self.A) if waves_per_state is None else int(waves_per_state)
        valid = torch.zeros((n, self.A), dtype=torch.uint8, device=dev)
        scores = torch.full((n, self.A, self.P), INT32_MIN, dtype=torch.int32, device=dev)
        ended = torch.zeros((n, self.A, self.P), dtype=torch.float32, device=dev)
        nxt = torch.full((n, self.A), -1, dtype=torch.int32, device=dev)
        states = torch.zeros((n, self.A, self.S), dtype=torch.int8, device=dev) if successor_states else None
        check(lib().azg_env_lookahead(self.GAME_ID, self.variant, _ptr(boards), _ptr(players), _ptr(active), n, W,
                                      C.c_uint64(int(self.rng_seed) & (2 ** 64 - 1)), C.c_uint64(int(stream0) & (2 ** 64 - 1)), _ptr(counters),
                                      _ptr(valid), _ptr(scores), _ptr(ended), _ptr(nxt), _ptr(states), _stream()))
        return Lookahead(valid, scores, ended, nxt, states)

    def max_symmetries(self):
        return {0: 10 + 2 * self.P, 1: 8, 2: 120, 3: 1, 4: 12, 5: 2 * self.P + 1, 6: 14, 7: 6, 8: 3}[self.GAME_ID]    # Splendor, Santorini, Azul, Minivilles, Abalone, TLP, Botanik, Akropolis, Smallworld

    def symmetries_batch(self, boards, pi, valids, max_sym=None, rng_seed=None, stream0=0):
        """getSymmetries for n (board int8[n,S], pi f32[n,A], valids u8[n,A]) triples on device ->
        (boards int8[n,K,S], pi f32[n,K,A], valids u8[n,K,A], count i32[n]), K = max_sym; rows >= count[t] are unspecified.
        Games whose symmetries are random (The Little Prince shuffles) draw triple t from stream (rng_seed, stream0 + t)."""
        n = boards.shape[0]
        K = max_sym or self.max_symmetries()
        boards = boards.reshape(n, -1)
        valids = valids if valids.dtype == torch.uint8 else valids.to(torch.uint8)
        assert boards.dtype == torch.int8 and pi.dtype == torch.float32
        assert boards.is_contiguous() and pi.is_contiguous() and valids.is_contiguous()
        ob = torch.empty((n, K, self.S), dtype=torch.int8, device=self.device)
        op = torch.empty((n, K, self.A), dtype=torch.float32, device=self.device)
        ov = torch.empty((n, K, self.A), dtype=torch.uint8, device=self.device)
        cnt = torch.zeros((n,), dtype=torch.int32, device=self.device)
        check(lib().azg_env_symmetries_ex(self.GAME_ID, self.variant, _ptr(boards), _ptr(pi), _ptr(valids), n, K, _ptr(ob), _ptr(op),
                                          _ptr(ov), _ptr(cnt), self.rng_seed if rng_seed is None else rng_seed, stream0, _stream()))
        return ob, op, ov, cnt

    # ---- Game.py API (numpy in / numpy out, one board) ----
    def _dev(self, board):
        return torch.from_numpy(np.ascontiguousarray(board, dtype=np.int8).reshape(1, self.S)).to(self.device)

    def _i32(self, v):
        return torch.tensor([int(v)], dtype=torch.int32, device=self.device)

    def getBoardSize(self):
        return ((5, 5, 3) if self.GAME_ID == _lib.SANTORINI else (9, 9, 4) if self.GAME_ID == _lib.ABALONE else (66, 5, 7) if self.GAME_ID == _lib.BOTANIK
                else (13, 13, self.cols) if self.GAME_ID == _lib.AKROPOLIS else (self.rows, self.cols))

    def getActionSize(self):
        return self.A

    def getNumberOfPlayers(self):
        return self.P

    def getInitBoard(self):
        self._stream_ctr += 1
        return self.init_boards_batch(1, stream0=self._stream_ctr)[0].cpu().numpy().reshape(self.getBoardSize())

    def getNextState(self, board, player, action, random_seed=0):
        seeds = torch.tensor([int(random_seed)], dtype=torch.int64, device=self.device)
        self._stream_ctr += 1
        out, nxt = self.next_state_batch(self._dev(board), self._i32(player), self._i32(action), seeds,
                                         stream0=(1 << 40) + self._stream_ctr)
        return out[0].cpu().numpy().reshape(self.getBoardSize()), int(nxt[0].item())

    def getValidMoves(self, board, player):
        return self.valid_moves_batch(self._dev(board), self._i32(player))[0].cpu().numpy().astype(bool)

    def getGameEnded(self, board, next_player):
        return self.game_ended_batch(self._dev(board), self._i32(next_player))[0][0].cpu().numpy()

    def getScore(self, board, player):
        return int(self.game_ended_batch(self._dev(board), self._i32(0))[1][0, player].item())

    def getRound(self, board):
        return int(self.game_ended_batch(self._dev(board), self._i32(0))[2][0].item())

    def getCanonicalForm(self, board, player):
        if player == 0:
            return board
        return self.canonical_batch(self._dev(board), self._i32(player))[0].cpu().numpy().reshape(self.getBoardSize())

    def getSymmetries(self, board, pi, valid_actions):
        """Game.getSymmetries (Game.py:96-109): list of (board, pi, valids) forms, identity first"""
        import numpy as np
        b = self._dev(board).reshape(1, -1)
        p = torch.as_tensor(np.asarray(pi, dtype=np.float32)).reshape(1, -1).to(self.device)
        v = torch.as_tensor(np.asarray(valid_actions).astype(np.uint8)).reshape(1, -1).to(self.device)
        self._stream_ctr += 1
        ob, op, ov, cnt = self.symmetries_batch(b, p, v, stream0=(1 << 41) + self._stream_ctr)
        k = int(cnt[0])
        shape = tuple(self.getBoardSize())
        ob, op, ov = ob[0, :k].cpu().numpy(), op[0, :k].cpu().numpy(), ov[0, :k].cpu().numpy().astype(bool)
        return [(ob[i].reshape(shape), op[i], ov[i]) for i in range(k)]

    def stringRepresentation(self, board):
        return np.ascontiguousarray(board, dtype=np.int8).tobytes()


class SplendorGame(HipGame):
    GAME_ID = _lib.SPLENDOR

    def __init__(self, num_players=2, **kw):
        super().__init__(num_players, **kw)


class SantoriniGame(HipGame):
    GAME_ID = _lib.SANTORINI

    def __init__(self, nb_gods=11, **kw):
        super().__init__(nb_gods, **kw)


class AzulGame(HipGame):
    GAME_ID = _lib.AZUL

    def __init__(self, **kw):
        super().__init__(2, **kw)


class MinivillesGame(HipGame):
    """minivilles/MinivillesGame.py (NUMBER_PLAYERS 2..4).  The env step rolls dice whatever random_seed says
    (MinivillesLogicNumba.py:232-242): every getNextState / getInitBoard draws from the engine's counter RNG stream."""
    GAME_ID = _lib.MINIVILLES

    def __init__(self, num_players=2, **kw):
        super().__init__(num_players, **kw)


ABALONE_LAYOUTS = ('classic', 'belgian', 'german')       # the reference's INITIAL_LAYOUT 0 / 1 / 2 (abalone/AbaloneLogicNumba.py:5)


def abalone_variant(layout='belgian', dynamic_komi=False):
    """(layout name or the reference's integer, ENABLE_DYNAMIC_KOMI) -> (layout name, bool, the C-ABI variant of include/azg.h: bits 0-1
    the layout -- 1 Belgian Daisy, 2 German Daisy, 3 classic -- and 4 for dynamic komi).  ValueError for anything else."""
    if isinstance(layout, str):
        name = layout.lower()
    elif isinstance(layout, (int, np.integer)) and not isinstance(layout, bool) and 0 <= layout < len(ABALONE_LAYOUTS):
        name = ABALONE_LAYOUTS[layout]
    else:
        name = None
    if name not in ABALONE_LAYOUTS:
        raise ValueError('Abalone layout %r: one of %s or 0 / 1 / 2' % (layout, ' / '.join(map(repr, ABALONE_LAYOUTS))))
    if not isinstance(dynamic_komi, (bool, np.bool_)):
        raise ValueError('Abalone dynamic_komi %r: True or False' % (dynamic_komi,))
    return name, bool(dynamic_komi), {'belgian': 1, 'german': 2, 'classic': 3}[name] | (4 if dynamic_komi else 0)


class AbaloneGame(HipGame):
    """abalone/AbaloneGame.py (2 players) for every value of the reference's two module constants (abalone/AbaloneLogicNumba.py:5-6):
    layout 'classic' | 'belgian' | 'german' (or its INITIAL_LAYOUT 0 / 1 / 2) and dynamic_komi (ENABLE_DYNAMIC_KOMI: getInitBoard draws
    who wins a score tie at the round limit into misc[0, 3], and there is no 0.001 draw).  The defaults are the shipped constants."""
    GAME_ID = _lib.ABALONE

    def __init__(self, layout='belgian', dynamic_komi=False, **kw):
        self.layout, self.dynamic_komi, variant = abalone_variant(layout, dynamic_komi)
        super().__init__(variant, **kw)


class TLPGame(HipGame):
    """thelittleprince/TLPGame.py (NUMBER_PLAYERS 3, 4 or 5).  The market refill inside the env step
    and getSymmetries draw true randomness (TLPLogicNumba.py:366-392, 177-272): both use the engine's counter RNG streams."""
    GAME_ID = _lib.TLP

    def __init__(self, num_players=3, **kw):
        super().__init__(num_players, **kw)


class BotanikGame(HipGame):
    """botanik/BotanikGame.py (2 players, MACHINE_SIZE = 7: the shipped constants).  Every card drawn inside the env step takes a
    uniform of the engine's counter RNG stream (BotanikLogicNumba.py:414-438)."""
    GAME_ID = _lib.BOTANIK

    def __init__(self, **kw):
        super().__init__(2, **kw)


class AkropolisGame(HipGame):
    """akropolis/AkropolisGame.py (N_PLAYERS 2 -- the shipped constant -- 3 or 4; 13 x 13 cities, N + 2 tiles on the construction site)"""
    GAME_ID = _lib.AKROPOLIS

    def __init__(self, num_players=2, **kw):
        super().__init__(num_players, **kw)


class SmallworldGame(HipGame):
    """smallworld/SmallworldGame.py (NUMBER_PLAYERS 2 -- the shipped constant -- 3 or 4, each with its own map).  getSymmetries draws two random
    score offsets (SmallworldLogicNumba.py:281-299) from the engine's counter RNG streams."""
    GAME_ID = _lib.SMALLWORLD

    def __init__(self, num_players=2, **kw):
        super().__init__(num_players, **kw)


def import_game(name, **kw):
    """GameSwitcher.import_game equivalent (GameSwitcher.py:15-24) for the games on the hot path."""
    if name == 'splendor':
        return SplendorGame(**kw)
    if name == 'santorini':
        return SantoriniGame(**kw)
    if name == 'azul':
        return AzulGame(**kw)
    if name == 'minivilles':
        return MinivillesGame(**kw)
    if name == 'abalone':
        return AbaloneGame(**kw)
    if name == 'thelittleprince':
        return TLPGame(**kw)
    if name == 'botanik':
        return BotanikGame(**kw)
    if name == 'akropolis':
        return AkropolisGame(**kw)
    if name == 'smallworld':
        return SmallworldGame(**kw)
    raise ValueError('game %r is not on the accelerated path' % name)
