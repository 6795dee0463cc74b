"""GPU: azg_env_playouts (csrc/playout.hip.h) -- random playouts to the end of the game in one launch -- against the ply-by-ply loop over
the entry points that are themselves pinned to the oracle: game_ended_batch, valid_moves_batch, arena.pick_actions (mode 0) and
next_state_batch, the pick and the env step sharing (stream0, counters) as the kernel's contract says.  Every comparison is exact."""
import ctypes as C
import functools

import pytest

pytestmark = pytest.mark.gpu

CASES = {
    'splendor2': ('SplendorGame', (2,)), 'splendor4': ('SplendorGame', (4,)), 'santorini1': ('SantoriniGame', (1,)),
    'santorini11': ('SantoriniGame', (11,)), 'azul': ('AzulGame', ()), 'minivilles3': ('MinivillesGame', (3,)),
    'abalone': ('AbaloneGame', ()), 'tlp4': ('TLPGame', (4,)), 'botanik': ('BotanikGame', ()), 'akropolis2': ('AkropolisGame', (2,)),
    'smallworld3': ('SmallworldGame', (3,)), 'minivilles2': ('MinivillesGame', (2,)),
}
WHOLE_GAMES = ['splendor2', 'splendor4', 'santorini1', 'santorini11', 'azul', 'minivilles3', 'abalone', 'tlp4', 'botanik', 'akropolis2',
               'smallworld3']
STREAM0 = 5000


@functools.lru_cache(maxsize=None)
def make_game(case):
    from azg_amd import games
    cls, args = CASES[case]
    return getattr(games, cls)(*args, rng_seed=77)


def loop(game, boards, cur, counters, s0, max_plies):
    """the yardstick: what azg_env_playouts promises, ply by ply, one launch per step -> dict of ended [n, P], plies, status, boards, cur,
    counters, actions [n, plies played by the longest row] (-1 where a row no longer played)"""
    import torch
    from azg_amd.arena import pick_actions
    n, dev = boards.shape[0], boards.device
    boards, cur, counters = boards.clone(), cur.clone(), counters.clone()
    live = torch.ones(n, dtype=torch.bool, device=dev)
    ended = torch.zeros((n, game.P), dtype=torch.float32, device=dev)
    plies = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    zeros = torch.zeros(n, dtype=torch.int64, device=dev)
    trace = []
    for ply in range(max_plies + 1):
        e, _, _ = game.game_ended_batch(boards, cur)
        fin = live & (e != 0).any(dim=1)
        ended = torch.where(fin[:, None], e, ended)
        live = live & ~fin
        if ply == max_plies:
            status = torch.where(live, torch.ones_like(status), status)
            break
        if not bool(live.any().item()):
            break
        valid = game.valid_moves_batch(boards, cur)
        stuck = live & (valid.sum(dim=1) == 0)
        status = torch.where(stuck, torch.full_like(status, 2), status)
        live = live & ~stuck
        if not bool(live.any().item()):
            break
        actions = torch.full((n,), -1, dtype=torch.int32, device=dev)
        pick_actions(0, None, valid, active=live, rng_seed=game.rng_seed, stream0=s0, counters=counters, out=actions)
        trace.append(actions.clone())
        # the env step of the live rows only: a row that no longer plays steps a copy of a live row's position and its result is dropped
        src = torch.where(live, torch.arange(n, device=dev), live.to(torch.int64).argmax())
        c2 = counters.clone()
        nb, ncur = game.next_state_batch(boards[src].contiguous(), cur[src].contiguous(), actions[src].contiguous(), zeros, stream0=s0, counters=c2)
        boards = torch.where(live[:, None], nb, boards)
        cur = torch.where(live, ncur, cur)
        counters = torch.where(live, c2, counters)
        plies = plies + live.to(torch.int32)
    acts = torch.stack(trace, dim=1) if trace else torch.zeros((n, 0), dtype=torch.int32, device=dev)
    return dict(ended=ended, plies=plies, status=status, boards=boards, cur=cur, counters=counters, actions=acts)


def start(case, n, s0=STREAM0):
    import torch
    g = make_game(case)
    counters = torch.zeros(n, dtype=torch.int64, device=g.device)
    boards = g.init_boards_batch(n, s0, counters)
    return g, boards, torch.zeros(n, dtype=torch.int32, device=g.device), counters


@functools.lru_cache(maxsize=None)
def whole_games(case):
    """five whole games of `case` by the loop, computed once and shared"""
    g, boards, cur, counters = start(case, 5)
    return g, boards, cur, counters, loop(g, boards, cur, counters, STREAM0, 4096)


def assert_same(out, counters, ref):
    import torch
    for name, got, want in (('ended', out.ended[:, 0], ref['ended']), ('plies', out.plies[:, 0], ref['plies']),
                            ('status', out.status[:, 0], ref['status']), ('boards', out.boards[:, 0], ref['boards']),
                            ('players', out.players[:, 0], ref['cur']), ('counters', counters, ref['counters'])):
        assert torch.equal(got, want), (name, got, want)
    L = ref['actions'].shape[1]
    assert torch.equal(out.actions[:, 0, :L], ref['actions']) and bool((out.actions[:, 0, L:] == -1).all().item())


def test_the_loop_reproduces_itself():
    import torch
    g, boards, cur, counters = start('minivilles2', 3)
    a, b = loop(g, boards, cur, counters, STREAM0, 4096), loop(g, boards, cur, counters, STREAM0, 4096)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert bool((a['plies'] > 0).all().item()) and not torch.equal(a['counters'], counters)


@pytest.mark.parametrize('case', WHOLE_GAMES)
def test_whole_games_equal_the_loop(case):
    g, boards, cur, counters, ref = whole_games(case)
    assert case == 'abalone' or bool((counters > 0).any().item())   # the streams go on where init_game left them (Abalone's set-up draws nothing)
    c = counters.clone()
    out = g.playouts_batch(boards, players=cur, k=1, max_plies=4096, stream0=STREAM0, counters=c, final_boards=True, trace=True)
    print(case, 'plies', ref['plies'].tolist(), 'status', ref['status'].tolist())
    assert bool((ref['status'] == 0).all().item()), 'a random game did not end within 4096 plies'
    assert_same(out, c, ref)


@pytest.mark.parametrize('case', ['splendor2', 'minivilles2'])
def test_cap(case):
    import torch
    g, boards, cur, counters = start(case, 3)
    ref = loop(g, boards, cur, counters, STREAM0, 5)
    c = counters.clone()
    out = g.playouts_batch(boards, players=cur, k=1, max_plies=5, stream0=STREAM0, counters=c, final_boards=True, trace=True)
    assert bool((out.status == 1).all().item()) and bool((out.plies == 5).all().item()) and bool((out.ended == 0).all().item())
    assert torch.equal(out.boards[:, 0], ref['boards']) and torch.equal(c, ref['counters']) and not torch.equal(c, counters)
    assert_same(out, c, ref)


@pytest.mark.parametrize('case', ['splendor2', 'abalone'])
def test_already_over(case):
    import torch
    g, _, _, _, ref = whole_games(case)
    keep = ref['status'] == 0
    assert bool(keep.any().item())
    boards, cur = ref['boards'][keep].contiguous(), ref['cur'][keep].contiguous()
    c0 = torch.arange(3, 3 + boards.shape[0], dtype=torch.int64, device=g.device)
    c = c0.clone()
    out = g.playouts_batch(boards, players=cur, k=1, max_plies=4096, stream0=9, counters=c, final_boards=True, trace=True)
    assert bool((out.plies == 0).all().item()) and bool((out.status == 0).all().item())
    assert torch.equal(out.ended[:, 0], g.game_ended_batch(boards, cur)[0]) and bool((out.ended != 0).any(dim=2).all().item())
    assert torch.equal(c, c0) and torch.equal(out.boards[:, 0], boards) and torch.equal(out.players[:, 0], cur)
    assert bool((out.actions == -1).all().item())


def sentinel_outputs(g, n, k, max_plies):
    import torch
    dev = g.device
    return dict(ended=torch.full((n, k, g.P), 7.0, dtype=torch.float32, device=dev), plies=torch.full((n, k), -5, dtype=torch.int32, device=dev),
                status=torch.full((n, k), 9, dtype=torch.uint8, device=dev), out_boards=torch.full((n, k, g.S), 111, dtype=torch.int8, device=dev),
                out_players=torch.full((n, k), -5, dtype=torch.int32, device=dev),
                out_actions=torch.full((n, k, max_plies), -7, dtype=torch.int32, device=dev))


@pytest.mark.parametrize('case', ['minivilles2', 'santorini1'])
def test_stream_layout_and_active(case):
    import torch
    from azg_amd.games import playouts_into
    g, boards, cur, counters = start(case, 3)
    # row t * k + j is playout j of board t: 2 boards x 3 playouts == the 6 boards, each repeated three times, x 1 playout
    c23 = counters[:2].repeat_interleave(3).contiguous()
    c61 = c23.clone()
    a = g.playouts_batch(boards[:2], players=cur[:2], k=3, max_plies=4096, stream0=40, counters=c23, final_boards=True, trace=True)
    b = g.playouts_batch(boards[:2].repeat_interleave(3, dim=0).contiguous(), players=cur[:2].repeat_interleave(3).contiguous(), k=1,
                         max_plies=4096, stream0=40, counters=c61, final_boards=True, trace=True)
    for x, y in zip(a, b):
        assert torch.equal(x.reshape((6,) + x.shape[2:]), y.reshape((6,) + y.shape[2:]))
    assert torch.equal(c23, c61)
    assert not torch.equal(a.actions[0, 0], a.actions[0, 1])                   # the playouts of one board are different games
    # active: the rows of board 1 keep what they held, the others do not notice it
    k, mp = 2, 512
    c_all = counters.repeat_interleave(k).contiguous()
    c_act = c_all.clone()
    full, part = sentinel_outputs(g, 3, k, mp), sentinel_outputs(g, 3, k, mp)
    playouts_into(g, boards, cur, k, mp, None, 40, c_all, **full)
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device=g.device)
    playouts_into(g, boards, cur, k, mp, active, 40, c_act, **part)
    fresh = sentinel_outputs(g, 3, k, mp)
    for name in full:
        assert torch.equal(part[name][1], fresh[name][1]), name
        assert torch.equal(part[name][0], full[name][0]) and torch.equal(part[name][2], full[name][2]), name
    assert torch.equal(c_act[k:2 * k], counters[1:2].repeat_interleave(k))
    assert torch.equal(c_act[:k], c_all[:k]) and torch.equal(c_act[2 * k:], c_all[2 * k:]) and not torch.equal(c_all[k:2 * k], c_act[k:2 * k])


def test_non_canonical_start():
    """Splendor with four players from ply 7 of the whole games above: the player to move is seat 3, the results stay in the seat numbering
    of the board"""
    import torch
    g, boards, cur, counters, ref = whole_games('splendor4')
    mid = loop(g, boards, cur, counters, STREAM0, 7)
    assert bool((mid['status'] == 1).all().item()) and bool((mid['cur'] != 0).all().item())
    assert torch.equal(mid['actions'], ref['actions'][:, :7])
    rest = loop(g, mid['boards'], mid['cur'], mid['counters'], STREAM0, 4096)
    c = mid['counters'].clone()
    out = g.playouts_batch(mid['boards'], players=mid['cur'], k=1, max_plies=4096, stream0=STREAM0, counters=c, final_boards=True, trace=True)
    assert_same(out, c, rest)
    # ... and it is the rest of the same games
    assert torch.equal(out.ended[:, 0], ref['ended']) and torch.equal(out.plies[:, 0] + 7, ref['plies']) and torch.equal(c, ref['counters'])


def test_errors_launch_nothing():
    import torch
    from azg_amd._lib import lib
    from azg_amd.games import _ptr, _stream
    g, boards, cur, counters = start('splendor2', 2)

    def call(game_id, n, k, max_plies, o, c):
        return lib().azg_env_playouts(game_id, g.variant, _ptr(boards), _ptr(cur), None, n, k, max_plies, C.c_uint64(1), C.c_uint64(0), _ptr(c),
                                      _ptr(o['ended']), _ptr(o['plies']), _ptr(o['status']), _ptr(o['out_boards']), _ptr(o['out_players']),
                                      _ptr(o['out_actions']), _stream())

    for game_id, k, max_plies in ((g.GAME_ID, 0, 16), (g.GAME_ID, 1, 0), (g.GAME_ID, 1, 70000), (99, 1, 16)):
        o, fresh, c = sentinel_outputs(g, 2, 1, 16), sentinel_outputs(g, 2, 1, 16), counters.clone()
        assert call(game_id, 2, k, max_plies, o, c) < 0 and lib().azg_last_error()
        torch.cuda.synchronize()
        assert all(torch.equal(o[name], fresh[name]) for name in o) and torch.equal(c, counters)
    o, fresh = sentinel_outputs(g, 2, 1, 16), sentinel_outputs(g, 2, 1, 16)
    assert call(g.GAME_ID, 0, 1, 16, o, counters.clone()) == 0
    assert lib().azg_env_playouts(g.GAME_ID, g.variant, None, None, None, 0, 1, 16, C.c_uint64(1), C.c_uint64(0), None, None, None, None, None,
                                  None, None, _stream()) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(o[name], fresh[name]) for name in o)
    o = sentinel_outputs(g, 2, 1, 16)
    o['status'] = None                                         # a required output
    assert call(g.GAME_ID, 2, 1, 16, o, counters.clone()) < 0
    with pytest.raises(Exception):
        g.playouts_batch(boards, k=0)
