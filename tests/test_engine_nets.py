"""The table of engine nets (nnet_wrapper.ENGINE_NETS) on the CPU: every versioned trainable module of azg_amd.train has exactly one
row, and the wrapper's (game, variant, version) -> module lookup and Coach's engine-module test are the table's."""
import inspect
from types import SimpleNamespace

import pytest
import torch

from azg_amd import _lib, nnet_wrapper, train

# a variant each game accepts, for the rows that accept any (the player count where the game has several)
VARIANT = {_lib.SPLENDOR: 2, _lib.AZUL: 2, _lib.ABALONE: 1, _lib.SMALLWORLD: 2, _lib.AKROPOLIS: 2, _lib.MINIVILLES: 2, _lib.TLP: 3,
           _lib.BOTANIK: 2}
ROWS = nnet_wrapper.ENGINE_NETS


def _game(gid, variant):
    _, A, P, _, _ = _lib.game_info(gid, variant)
    return SimpleNamespace(GAME_ID=gid, P=P, A=A, variant=variant, device=torch.device('cpu'))


def _row_game(row):
    return _game(row.game, row.variants[0] if row.variants else VARIANT[row.game])


def test_every_versioned_module_has_exactly_one_row():
    mods = [c for _, c in inspect.getmembers(train, inspect.isclass)
            if c.__module__ == train.__name__ and issubclass(c, torch.nn.Module) and hasattr(c, 'version')]
    assert len(mods) >= 11
    for c in mods:
        assert [r.module for r in ROWS].count(c) == 1, c.__name__
    assert {r.module for r in ROWS} == set(mods)


@pytest.mark.parametrize('row', ROWS, ids=lambda r: r.module.__name__)
def test_module_for_builds_the_row_module(row):
    g = _row_game(row)
    m = nnet_wrapper._module_for(g, row.version, 0.0)
    assert type(m) is row.module and m.version == row.version and (m.P, m.A) == (g.P, g.A)
    assert nnet_wrapper.is_engine_module(m)
    for ver in (row.version + 1000, None):
        with pytest.raises(ValueError):
            nnet_wrapper._module_for(g, ver, 0.0)


def test_santorini_versions_follow_the_variant():
    """89 is the no-gods net (variant 1), 78 the with-gods net (variant 11); the other pairings raise"""
    for variant, built, other in ((1, 89, 78), (11, 78, 89)):
        g = _game(_lib.SANTORINI, variant)
        assert nnet_wrapper._module_for(g, built, 0.0).version == built
        with pytest.raises(ValueError):
            nnet_wrapper._module_for(g, other, 0.0)


def test_engine_module_lookup_follows_the_mro():
    """V11 (a subclass of V10) finds its own row; a user's subclass of an engine module keeps the engine net; a plain torch module
    has none"""
    assert nnet_wrapper._engine_net(train.BotanikV11Module(2, 428, 0.0)).version == 11

    class Mine(train.BotanikV10Module):
        pass
    assert nnet_wrapper._engine_net(Mine(2, 428, 0.0)).module is train.BotanikV10Module
    assert not nnet_wrapper.is_engine_module(torch.nn.Linear(2, 2))
    assert not nnet_wrapper.is_engine_module(torch.nn.Module())
