"""CPU: the Python table of the asynchronous tree pipeline (azg_amd.forest.PIPELINE_ROWS) and its eligibility function, driven with stub
evaluators -- plain objects with the attributes the real ones carry.  The expected outcomes below are literals, recorded from the six
hand-kept `can_*` expressions that SelfPlayEngine.__init__ held before the table replaced them; nothing here is derived from the table."""
import pytest
import torch

from azg_amd import _lib
from azg_amd.forest import NET_HASH, NET_MB1D, NET_SW62, NET_V80, NET_V89, PIPELINE_ROWS, pipeline_needs, pipeline_row

T, A = 8, 30
SPLENDOR, SANTORINI, AZUL, MINIVILLES, ABALONE, TLP, SMALLWORLD = 0, 1, 2, 3, 4, 5, 8


def _stub(cls, **attrs):
    o = type(cls, (), {})()
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def _pi(t=T, a=A):
    return torch.empty((t, a))


def v80(**kw):
    return _stub('SplendorV80Hip', **dict(dict(h2=True, fused_net=True, net_ptrs_h2=object(), descale_h2=object(), pi=_pi()), **kw))


def v89(**kw):
    return _stub('SantoriniV89Hip', **dict(dict(h2=True, ptrs=object(), descale=1.0, pi=_pi()), **kw))


def mb(geometry, **kw):
    return _stub('MobileNet1dHip', **dict(dict(h2=True, fused=True, geometry=geometry, fused_ptrs_h2=object(), descale_h2=object(), pi=_pi()), **kw))


def sw62(**kw):
    return _stub('SmallworldV62Hip', **dict(dict(ptrs=object(), pi=_pi()), **kw))


def hashnet():
    return _stub('HashNetPipeline', async_hashnet=True)


# (game, variant) -> (the row's name, on by default, the engine net it takes, that net's C entry point, a net of the family with the WRONG
# geometry or None where the family has no geometry)
EXPECT = {
    (SPLENDOR, 0): ('Splendor 2 players', True, v80, 'azg_forest_async_rounds_v80_h2', None),
    (SPLENDOR, 2): ('Splendor 2 players', True, v80, 'azg_forest_async_rounds_v80_h2', None),
    (SPLENDOR, 3): ('Splendor 3 / 4 players', True, lambda **kw: mb(1, **kw), 'azg_forest_async_rounds_mb1d_h2', lambda: mb(2)),
    (SPLENDOR, 4): ('Splendor 3 / 4 players', True, lambda **kw: mb(2, **kw), 'azg_forest_async_rounds_mb1d_h2', lambda: mb(1)),
    (SANTORINI, 1): ('Santorini no-gods', True, v89, 'azg_forest_async_rounds_conv5_h2', None),
    (AZUL, 0): ('Azul', True, lambda **kw: mb(3, **kw), 'azg_forest_async_rounds_mb1d_h2', lambda: mb(0)),
    (AZUL, 2): ('Azul', True, lambda **kw: mb(3, **kw), 'azg_forest_async_rounds_mb1d_h2', lambda: mb(4)),
    (SMALLWORLD, 2): ('Smallworld 2 - 4 players', False, sw62, 'azg_forest_async_rounds_sw62', None),
    (SMALLWORLD, 3): ('Smallworld 2 - 4 players', False, sw62, 'azg_forest_async_rounds_sw62', None),
    (SMALLWORLD, 4): ('Smallworld 2 - 4 players', False, sw62, 'azg_forest_async_rounds_sw62', None),
    (MINIVILLES, 2): ('Minivilles 2 - 4 players', False, lambda **kw: mb(4, **kw), 'azg_forest_async_rounds_mb1d_h2', lambda: mb(6)),
    (MINIVILLES, 3): ('Minivilles 2 - 4 players', False, lambda **kw: mb(6, **kw), 'azg_forest_async_rounds_mb1d_h2', lambda: mb(7)),
    (MINIVILLES, 4): ('Minivilles 2 - 4 players', False, lambda **kw: mb(7, **kw), 'azg_forest_async_rounds_mb1d_h2', lambda: mb(4)),
    (TLP, 3): ('The Little Prince 3 - 5 players', False, lambda **kw: mb(5, **kw), 'azg_forest_async_rounds_mb1d_h2', lambda: mb(4)),
    (TLP, 4): ('The Little Prince 3 - 5 players', False, lambda **kw: mb(8, **kw), 'azg_forest_async_rounds_mb1d_h2', lambda: mb(5)),
    (TLP, 5): ('The Little Prince 3 - 5 players', False, lambda **kw: mb(9, **kw), 'azg_forest_async_rounds_mb1d_h2', lambda: mb(8)),
}
# forests the pipeline does not run, whatever the evaluator
NOT_SERVED = [(SPLENDOR, 5), (SANTORINI, 0), (SANTORINI, 11), (SMALLWORLD, 5), (MINIVILLES, 5), (MINIVILLES, 0), (TLP, 2), (TLP, 0), (ABALONE, 0)]
ALL_NETS = [v80, v89, sw62, hashnet] + [(lambda g: lambda: mb(g))(g) for g in range(10)]


def _row(game, variant, nets, fused=True, trees=T, a=A):
    return pipeline_row(game, variant, fused, nets, trees, a)


def test_the_ids_are_the_librarys():
    assert (SPLENDOR, SANTORINI, AZUL, MINIVILLES, ABALONE, TLP, SMALLWORLD) == (
        _lib.SPLENDOR, _lib.SANTORINI, _lib.AZUL, _lib.MINIVILLES, _lib.ABALONE, _lib.TLP, _lib.SMALLWORLD)


@pytest.mark.parametrize('game,variant', sorted(EXPECT))
def test_row_of_every_game_and_variant(game, variant):
    name, default_on, right, entry, wrong_geometry = EXPECT[(game, variant)]
    # the right net, and the tests' hash-net: the same row, on by default or opt-in
    for nets in ([right()], [hashnet()], [right(), right()], [hashnet(), hashnet()]):
        row = _row(game, variant, nets)
        assert row is not None and row.name == name and row.default_on is default_on, (game, variant, nets)
    assert _row(game, variant, [right()]).net.entry == entry
    # every evaluator of another family or another geometry, a mix, the torch net: no row
    for mk in ALL_NETS:
        n = mk()
        same = type(n).__name__ == type(right()).__name__ and getattr(n, 'geometry', None) == getattr(right(), 'geometry', None)
        if not same and not getattr(n, 'async_hashnet', False):
            assert _row(game, variant, [n]) is None, (game, variant, type(n).__name__, getattr(n, 'geometry', None))
            assert _row(game, variant, [right(), n]) is None
    assert _row(game, variant, [right(), hashnet()]) is None
    assert _row(game, variant, [_stub('SplendorV80')]) is None
    if wrong_geometry is not None:
        assert _row(game, variant, [wrong_geometry()]) is None
        n = right()
        n.geometry = None
        assert _row(game, variant, [n]) is None
    # static output buffers of another shape, or none
    assert _row(game, variant, [right(pi=_pi(2 * T, A))]) is None
    assert _row(game, variant, [right(pi=_pi(T, A + 1))]) is None
    assert _row(game, variant, [right(pi=None)]) is None
    assert _row(game, variant, [right()], trees=T // 2) is None
    assert _row(game, variant, [right()], a=A - 1) is None
    # the lock-step rounds that are not the fused ones: no pipeline, not with the hash-net either
    assert _row(game, variant, [right()], fused=False) is None
    assert _row(game, variant, [hashnet()], fused=False) is None


def test_flags_the_evaluators_must_carry():
    assert _row(SPLENDOR, 2, [v80(h2=False)]) is None and _row(SPLENDOR, 2, [v80(fused_net=False)]) is None
    n = v80()
    del n.net_ptrs_h2
    assert _row(SPLENDOR, 2, [n]) is None
    # the V80 row knows its evaluator by attributes, the others by class name
    assert _row(SPLENDOR, 2, [_stub('AnotherName', h2=True, fused_net=True, net_ptrs_h2=object(), pi=_pi())]).name == 'Splendor 2 players'
    assert _row(SANTORINI, 1, [v89(h2=False)]) is None
    assert _row(SANTORINI, 1, [_stub('AnotherName', h2=True, ptrs=object(), pi=_pi())]) is None
    assert _row(SPLENDOR, 3, [mb(1, h2=False)]) is None and _row(SPLENDOR, 3, [mb(1, fused=False)]) is None
    assert _row(MINIVILLES, 2, [mb(4, h2=False)]) is None and _row(TLP, 3, [mb(5, fused=False)]) is None
    assert _row(SMALLWORLD, 2, [_stub('SmallworldV62', pi=_pi())]) is None


@pytest.mark.parametrize('game,variant', NOT_SERVED)
def test_forests_without_a_row(game, variant):
    for mk in ALL_NETS:
        assert _row(game, variant, [mk()]) is None, (game, variant)


def test_default_on_and_opt_in_rows():
    on = sorted(r.name for r in PIPELINE_ROWS if r.default_on)
    opt = sorted(r.name for r in PIPELINE_ROWS if not r.default_on)
    assert on == ['Azul', 'Santorini no-gods', 'Splendor 2 players', 'Splendor 3 / 4 players']
    assert opt == ['Minivilles 2 - 4 players', 'Smallworld 2 - 4 players', 'The Little Prince 3 - 5 players']
    assert {r.net for r in PIPELINE_ROWS} == {NET_V80, NET_V89, NET_MB1D, NET_SW62} and NET_HASH.entry == 'azg_forest_async_rounds_hashnet'


def test_unsupported_async_pipe_is_a_value_error():
    """async_pipe=True with what the pipeline cannot run is refused before anything is made on the GPU; the text lists what it can run"""
    from azg_amd.selfplay import SelfPlayEngine
    game = lambda g, v: _stub('Game', GAME_ID=g, variant=v, device='cuda:0')  # noqa: E731
    a2 = _lib.game_info(SPLENDOR, 2)[1]
    for g, v, net, groups in ((SPLENDOR, 2, _stub('SplendorV80'), 1),                       # the torch net
                              (SPLENDOR, 2, v80(pi=_pi(T, a2 + 1)), 1),                     # static buffers of another shape
                              (SPLENDOR, 2, [v80(pi=_pi(T // 2, a2)), v80(pi=_pi(T // 2, a2))], 2),      # two groups
                              (MINIVILLES, 2, mb(5, pi=_pi(T, _lib.game_info(MINIVILLES, 2)[1])), 1),   # a TLP net on a Minivilles engine
                              (SANTORINI, 11, hashnet(), 1), (ABALONE, 0, hashnet(), 1)):  # no descent kernel
        with pytest.raises(ValueError) as e:
            SelfPlayEngine(game(g, v), net, {}, T, groups=groups, async_pipe=True)
        msg = str(e.value)
        assert msg == pipeline_needs() and msg.startswith('async_pipe=True needs ') and 'groups == 1' in msg and 'hash-net' in msg
        for word in ('Splendor 2 players', 'SplendorV80Hip(h2=True)', 'Santorini no-gods', 'SantoriniV89Hip(h2=True)', 'Splendor 3 / 4 players',
                     'Azul', 'Minivilles 2 - 4 players', 'The Little Prince 3 - 5 players', 'MobileNet1dHip(h2=True)', 'Smallworld 2 - 4 players',
                     'SmallworldV62Hip', 'max_batch == n_games'):
            assert word in msg, word
    # percu=True keeps its own refusal
    with pytest.raises(ValueError, match='percu=True needs Splendor 2 players'):
        SelfPlayEngine(game(SPLENDOR, 3), mb(1, pi=_pi(T, _lib.game_info(SPLENDOR, 3)[1])), {}, T, percu=True)
