"""Arena.playGames on the engine (Arena.py:35-140, pit.py:26-66): N head-to-head games run concurrently, one search tree
per game and per contestant, every ply one batched MCTS per contestant over the games where it is to move.

The reference's own Arena only needs the duck-typed surface, so `Arena.Arena(player1, player2, azg_amd.games.SplendorGame())`
with `azg_amd.mcts.MCTS`-based players already works unchanged (one game at a time); this class is the batched form:
  * seats alternate 1-2-2-1 over the games (Arena.py:121-125): game i is "one vs two" when i % 4 in (0, 3); with more than
    two players the first seat belongs to one contestant and all other seats to the other (Arena.py:52-55);
  * a contestant = (nnet, args): its move is argmax_a of getActionProb(canonical, temp=temp_for_game(turn),
    force_full_search=True) (Coach.py:193-194, pit.py:60-64): above 0.02 the temperature only sharpens the visit counts and the
    argmax is the most visited action (first index on ties, np.argmax); once temp_for_game(turn) <= 0.02 (late in long games)
    getActionProb itself returns a one-hot on a maximum drawn at random among ties (MCTS.py:93-98; the tree's counter RNG);
  * the real move uses random_seed = 0 (Arena.py:84) -- the engine's counter-based RNG stream of that game;
  * the result of a game is getGameEnded(board, curPlayer)[0] (Arena.py:101), tallied like playGames (:126-131).

Baselines (pit.py's players, <G>Players.py): instead of an nnet a contestant may be a RandomContestant() -- <G>Players.RandomPlayer.play,
uniform among the valid moves -- or a PolicyContestant(nnet) -- the net's policy without a search.  Neither owns a forest; their move
is one launch of azg_pick_actions (csrc/pick.hip.h) on the [T, A] rows of the ply.  vs_random(...) is the pit-style call.
GreedyContestant(rule) -- <G>Players.GreedyPlayer.play -- is a third baseline: a one-ply lookahead (csrc/lookahead.hip.h) narrows the valid
moves to the rule's candidates before the same pick; vs_greedy(...) is `pit.py <game> greedy <checkpoint>`.
nnet.RolloutEvaluator in the place of an nnet makes a contestant a pure MCTS (uniform prior, random playouts as the leaf value), and
random_games(...) plays whole random games in one launch (csrc/playout.hip.h)."""
import ctypes as C

import torch

from . import _lib
from ._lib import check, lib
from .games import GREEDY_RULES, _ptr, _stream, greedy_candidates
from .mcts import BatchedMCTS

PICK_UNIFORM, PICK_ARGMAX, PICK_SAMPLE = 0, 1, 2


def pick_actions(mode, probs, valid, active=None, rng_seed=0, stream0=0, counters=None, out=None):
    """azg_pick_actions (include/azg.h) on CUDA tensors: one action per row of probs f32[T, A] / valid u8[T, A] (either may be None where
    the mode allows it).  mode 0: uniform among the valid actions; 1: first-index argmax of probs over them; 2: sampled proportionally to
    probs over them.  Modes 0 and 2 draw from (rng_seed, stream0 + row, counters[row]) and advance counters (int64[T]) by one.  Rows with
    active == 0 keep what `out` (int32[T], zeros when not given) holds and their counter.  -> out"""
    ref = probs if probs is not None else valid
    assert ref is not None, 'pick_actions needs probs or valid for the shape of the rows'
    T, A = ref.shape
    for x, dt in ((probs, (torch.float32,)), (valid, (torch.uint8, torch.bool)), (active, (torch.uint8, torch.bool))):
        assert x is None or (x.dtype in dt and x.is_contiguous() and x.device == ref.device), 'pick_actions: dtype / layout of an argument'
    assert (probs is None or valid is None or probs.shape == valid.shape) and (active is None or active.shape == (T,))
    assert counters is None or (counters.dtype == torch.int64 and counters.shape == (T,) and counters.is_contiguous())
    if out is None:
        out = torch.zeros(T, dtype=torch.int32, device=ref.device)
    assert out.dtype == torch.int32 and out.shape == (T,) and out.is_contiguous()
    check(lib().azg_pick_actions(int(mode), _ptr(probs), _ptr(valid), T, A, _ptr(active), C.c_uint64(int(rng_seed) & (2 ** 64 - 1)),
                                 C.c_uint64(int(stream0) & (2 ** 64 - 1)), _ptr(counters), _ptr(out), _stream()))
    return out


class RandomContestant:
    """<G>Players.RandomPlayer.play as an arena contestant: uniform among getValidMoves(canonical, 0)"""
    mode = PICK_UNIFORM

    def probs_valid(self, game, canonical):
        return None, game.valid_moves_batch(canonical, None)


class GreedyContestant:
    """<G>Players.GreedyPlayer.play as an arena contestant: a one-ply lookahead.  Per ply: every successor of every board in one launch
    (games.HipGame.lookahead_batch, csrc/lookahead.hip.h), the candidate moves of the rule (games.greedy_candidates), and the move uniform
    among them -- the pick of RandomContestant with the candidates in the place of the valid moves: same kernel, same stream
    stream0 + (c + 1) << 30 + i of game i, one draw per move.
    rule='reference': the reference's player, quirks included (include/azg.h, azg_greedy_candidates) -- Splendor, Azul (from the board
    alone: no lookahead) and Abalone; the reference's other six games define no greedy rule and raise.  rule='lead': this project's own
    rule for any game, the moves after which the mover's score leads the best other seat's by most.
    The lookahead of game i peeks at the env step's draws on a stream of its own, arena stream0 + 3 << 30 + i, always from counter 0
    (it collides with neither the arena's env stream stream0 + i nor the two pick streams); like RandomContestant's, game i's moves are a
    function of rng_seed and i, whatever n_parallel and however the match is dealt out."""
    mode = PICK_UNIFORM
    NO_RULE = 'azg_greedy_candidates: the reference defines no greedy player for this game'

    def __init__(self, rule='reference'):
        if rule not in GREEDY_RULES:
            raise ValueError("GreedyContestant: rule is 'reference' or 'lead', not %r" % (rule,))
        self.rule, self.peek_stream0 = rule, 3 * (1 << 30)

    def begin_wave(self, arena_stream0, first_game_index):
        self.peek_stream0 = arena_stream0 + 3 * (1 << 30) + first_game_index

    def probs_valid(self, game, canonical):
        if self.rule == 'reference' and game.GAME_ID not in (_lib.SPLENDOR, _lib.AZUL, _lib.ABALONE):
            raise _lib.AzgError(self.NO_RULE)
        if self.rule == 'reference' and game.GAME_ID == _lib.AZUL:
            return None, greedy_candidates(game, self.rule, canonical, game.valid_moves_batch(canonical, None), None)
        ahead = game.lookahead_batch(canonical, stream0=self.peek_stream0)
        return None, greedy_candidates(game, self.rule, canonical, ahead.valid, ahead.scores)


class PolicyContestant:
    """the raw policy of `nnet` as an arena contestant: one predict_batch per ply (all T rows of the wave: a fixed batch shape, rows of
    games where the contestant is not to move are ignored), then the first-index argmax over the valid moves, or with sample=True a move
    drawn proportionally to the policy (np.random.choice(A, p=pi))"""

    def __init__(self, nnet, sample=False):
        if not hasattr(nnet, 'predict_batch'):
            raise TypeError('PolicyContestant needs a net with predict_batch(boards, valids)')
        self.nnet, self.mode = nnet, PICK_SAMPLE if sample else PICK_ARGMAX

    def probs_valid(self, game, canonical):
        valid = game.valid_moves_batch(canonical, None)
        pi, _ = self.nnet.predict_batch(canonical.view((canonical.shape[0],) + tuple(game.getBoardSize())), valid.bool())
        return pi.float().contiguous(), valid


class BatchedArena:
    def __init__(self, game, nnet1, nnet2, args1, args2=None, n_parallel=64, node_capacity=None, stream0=0, temp_for_game=None,
                 first_game_index=0):
        """temp_for_game(turn) -> temperature of getActionProb at that turn (Coach.temp_for_game, Coach.py:273-276, or pit.py's
        variant); None = 1 at every turn (plain argmax of the visit counts).  first_game_index: index of the game tree 0 plays when
        a match is dealt out over several ranks -- the trees' own random streams (ties at temperature <= 0.02) follow the game index"""
        self.game, self.T, self.stream0 = game, n_parallel, stream0
        self.temp_for_game = temp_for_game
        kw = [dict(rng_seed=int(getattr(game, 'rng_seed', 0)), stream0=stream0 + (c + 1) * (1 << 30) + first_game_index) for c in (0, 1)]
        # a contestant is a search (BatchedMCTS on its own forest) or a baseline object; self.mcts lists the searches only
        self.contestants = [n if isinstance(n, (RandomContestant, PolicyContestant, GreedyContestant)) else
                            BatchedMCTS(game, n, a, n_parallel, node_capacity=node_capacity, **kw[c])
                            for c, (n, a) in enumerate(((nnet1, args1), (nnet2, args2 if args2 is not None else args1)))]
        self.mcts = [m for m in self.contestants if isinstance(m, BatchedMCTS)]
        self.max_plies = 4096

    def play_wave(self, first_game_index=0, n_games=None, record=None):
        """plays games [first_game_index, first_game_index + n_games) concurrently (n_games <= n_parallel);
        returns results f32[n_games] = getGameEnded(...)[0] per game and the bool 'one_vs_two' seating per game"""
        g, T, dev = self.game, self.T, self.game.device
        n = T if n_games is None else n_games
        idx = torch.arange(T, device=dev) + first_game_index
        one_vs_two = ((idx % 4 == 0) | (idx % 4 == 3))
        counters = torch.zeros(T, dtype=torch.int64, device=dev)
        boards = g.init_boards_batch(T, stream0=self.stream0 + first_game_index, counters=counters)
        cur = torch.zeros(T, dtype=torch.int32, device=dev)
        done = torch.arange(T, device=dev) >= n
        result = torch.zeros(T, dtype=torch.float32, device=dev)
        zero_seed = torch.zeros(T, dtype=torch.int64, device=dev)
        for m in self.mcts:
            m.reset_all_search_trees()                                       # Arena.py:99
        # a baseline contestant draws game i's moves from a stream of its own, stream0 + (c + 1) << 30 + i, from counter 0: a function of the
        # game index only, whatever n_parallel and however the match is dealt out
        pick_counters = [None if isinstance(m, BatchedMCTS) else torch.zeros(T, dtype=torch.int64, device=dev) for m in self.contestants]
        for m in self.contestants:                                           # (a lookahead contestant's peek stream follows the game index too)
            if hasattr(m, 'begin_wave'):
                m.begin_wave(self.stream0, first_game_index)
        for ply in range(self.max_plies):
            if bool(done.all().item()):
                break
            # seat 0 belongs to contestant 0 in a "one vs two" game, to contestant 1 otherwise; other seats to the other one
            owner = torch.where((cur == 0) == one_vs_two, torch.zeros_like(cur), torch.ones_like(cur))
            canonical = g.canonical_batch(boards, cur)
            actions = torch.zeros(T, dtype=torch.int32, device=dev)
            for c, m in enumerate(self.contestants):
                active = (~done) & (owner == c)
                if not bool(active.any().item()):
                    continue
                if pick_counters[c] is not None:
                    probs, valid = m.probs_valid(g, canonical)
                    pick_actions(m.mode, probs, valid, active, rng_seed=int(getattr(g, 'rng_seed', 0)),
                                 stream0=self.stream0 + (c + 1) * (1 << 30) + first_game_index, counters=pick_counters[c], out=actions)
                    continue
                full = torch.where(active, torch.ones(T, dtype=torch.uint8, device=dev), torch.full((T,), 2, dtype=torch.uint8, device=dev))
                temp = 1 if self.temp_for_game is None else self.temp_for_game(ply + 1)       # `it` of Arena.py:67-68
                probs, _, _ = m.getActionProb(canonical, temp=temp, full=full)
                ar = torch.arange(probs.shape[1], device=dev)[None, :]              # np.argmax: FIRST index of the maximum
                first_max = torch.where(probs == probs.max(dim=1, keepdim=True).values, ar, probs.shape[1]).min(dim=1).values
                first_max = torch.where(first_max >= probs.shape[1], torch.zeros_like(first_max), first_max)   # all-NaN row -> 0, like np.argmax
                actions = torch.where(active, first_max.to(torch.int32), actions)
            if record is not None:
                record.append((boards.clone(), cur.clone(), actions.clone(), done.clone()))
            nb, ncur = g.next_state_batch(boards, cur, actions, zero_seed, stream0=self.stream0 + first_game_index, counters=counters)
            live = ~done
            boards = torch.where(live[:, None], nb, boards)
            cur = torch.where(live, ncur, cur)
            ended, _, _ = g.game_ended_batch(boards, cur)
            fin = live & (ended != 0).any(dim=1)
            result = torch.where(fin, ended[:, 0], result)
            done = done | fin
        return result[:n], one_vs_two[:n]

    def playGames(self, num, first_game_index=0):
        """-> (oneWon, twoWon, draws) like Arena.playGames (Arena.py:103-140).  first_game_index: this object plays games
        [first_game_index, first_game_index + num) of a match that is dealt out over several ranks (the seating and the random
        streams of a game are functions of its index)"""
        one = two = draws = 0
        for first in range(first_game_index, first_game_index + num, self.T):
            n = min(self.T, first_game_index + num - first)
            res, ovt = self.play_wave(first, n)
            win_first_seat, win_other = res == 1.0, res == -1.0
            one += int(((ovt & win_first_seat) | (~ovt & win_other)).sum().item())
            two += int(((ovt & win_other) | (~ovt & win_first_seat)).sum().item())
            draws += int((~(win_first_seat | win_other)).sum().item())
        return one, two, draws


def vs_random(game, nnet, args, num, **kw):
    """pit.py's first question of a net: `num` games of (nnet, args) with its search against RandomContestant, seats alternating as in
    playGames -> (won, lost, draws) from the net's side.  kw: BatchedArena's (n_parallel defaults to min(num, 64))"""
    kw.setdefault('n_parallel', max(1, min(int(num), 64)))
    return BatchedArena(game, nnet, RandomContestant(), args, **kw).playGames(num)


def vs_greedy(game, nnet, args, num, rule='reference', **kw):
    """pit.py's second question of a net (`pit.py <game> greedy <checkpoint>`): `num` games of (nnet, args) with its search against
    GreedyContestant(rule), seats alternating as in playGames -> (won, lost, draws) from the net's side.  kw: BatchedArena's (n_parallel
    defaults to min(num, 64))"""
    kw.setdefault('n_parallel', max(1, min(int(num), 64)))
    return BatchedArena(game, nnet, GreedyContestant(rule), args, **kw).playGames(num)


def random_games(game, num, stream0=0, max_plies=4096):
    """`num` games of uniformly random play from Board.init_game to the end, in two launches (launcher.py's random play; BatchedArena with two
    RandomContestants pays half a dozen launches and a host round trip per ply): init_boards_batch on streams stream0 .. stream0 + num - 1, then
    one playout per board on the same streams from the counters the init left.  Game i is a function of (game.rng_seed, stream0 + i) alone.
    -> (ended f32[num, P] = getGameEnded(final board, final player), plies i32[num], status u8[num]: 0 finished, 1 max_plies reached, 2 no
    valid move; ended is zero for 1 and 2)"""
    counters = torch.zeros(num, dtype=torch.int64, device=game.device)
    boards = game.init_boards_batch(num, stream0, counters)
    out = game.playouts_batch(boards, k=1, max_plies=max_plies, stream0=stream0, counters=counters)
    return out.ended[:, 0, :], out.plies[:, 0], out.status[:, 0]
