"""CPU-only: the surface of the validation losses -- azg_eval_losses declared in include/azg.h, exported by the built library and bound by
_lib.py; nnet.eval_losses / nnet.evaluate_examples, NNetWrapper.evaluate / evaluate_details, train.train's on_step hook, and the flags of
tools/train_offline.py (the reference's offline trainer, GenericNNetWrapper.py:353-367) with the reference's defaults."""
import ctypes
import importlib.util
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'alpha-zero-general_amd', 'libazg_hip.so')


def signature(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_eval_losses_is_declared_exported_and_bound():
    from azg_amd import _lib
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'azg.h')).read(), flags=re.S)
    m = re.search(r'\bint\s+azg_eval_losses\s*\(([^;]*)\)\s*;', h)
    assert m, 'include/azg.h does not declare azg_eval_losses'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    assert [p.split()[-1].lstrip('*') for p in params] == [
        'pi_dev', 'v_dev', 'target_pi_dev', 'z_dev', 'q_dev', 'active_dev', 'B', 'A', 'P', 'q_weight', 'rows_dev', 'flags_dev', 'totals_dev',
        'accumulate', 'stream'], params
    assert 'float q_weight' in params and 'double* rows_dev' in params and 'int32_t* flags_dev' in params and 'double* totals_dev' in params
    assert 'azg_eval_losses' in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(LIB), 'azg_eval_losses')
    at = _lib.lib().azg_eval_losses.argtypes
    assert len(at) == 15 and at[9] is ctypes.c_float


def test_python_surface():
    from azg_amd import nnet, nnet_wrapper, train
    empty = inspect.Parameter.empty
    assert signature(nnet.eval_losses) == [('pi', empty), ('v', empty), ('target_pi', empty), ('z', empty), ('q', empty), ('q_weight', empty),
                                           ('active', None), ('totals', None), ('accumulate', False)]
    assert signature(nnet.evaluate_examples) == [('evaluator', empty), ('cols', empty), ('q_weight', empty), ('batch', 4096)]
    W = nnet_wrapper.NNetWrapper
    assert signature(W.evaluate) == [('self', empty), ('validation_set', empty)]
    assert signature(W.evaluate_details)[:2] == [('self', empty), ('validation_set', empty)]
    assert signature(W.train)[:5] == [('self', empty), ('examples', empty), ('validation_set', None), ('save_folder', None), ('every', 0)]
    sig = signature(train.train)
    assert sig[-1] == ('on_step', None), sig
    assert sig[:3] == [('module', empty), ('examples', empty), ('learn_rate', 3e-3)]


def test_offline_trainer_flags_are_the_reference_s():
    spec = importlib.util.spec_from_file_location('train_offline', os.path.join(ROOT, 'tools', 'train_offline.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = mod.build_parser()
    flags = {a.dest: a for a in parser._actions if a.dest != 'help'}
    # GenericNNetWrapper.py:354-366: dest -> (option strings, default, type)
    want = {'game': ([], 'splendor', None), 'input': (['--input', '-i'], None, None), 'output': (['--output', '-o'], None, None),
            'training': (['--training', '-T'], None, None), 'test': (['--test', '-t'], None, None),
            'learn_rate': (['--learn-rate', '-l'], 0.0003, float), 'dropout': (['--dropout', '-d'], 0.3, float),
            'epochs': (['--epochs', '-p'], 2, int), 'batch_size': (['--batch-size', '-b'], 32, int),
            'nb_samples': (['--nb-samples', '-N'], 9999, int), 'nn_version': (['--nn-version', '-V'], -1, int),
            'q_weight': (['--q-weight', '-q'], 0.5, float)}
    for dest, (opts, default, typ) in want.items():
        a = flags[dest]
        assert sorted(a.option_strings) == sorted(opts) and a.default == default and a.type is typ, (dest, a)
    assert set(flags) - set(want) == {'num_players', 'variant'}
    ns = parser.parse_args(['minivilles', '-T', 'x.examples', '-b', '64', '-p', '1', '-V', '82', '--num-players', '3'])
    assert (ns.game, ns.training, ns.batch_size, ns.epochs, ns.nn_version, ns.num_players, ns.test, ns.input) == (
        'minivilles', 'x.examples', 64, 1, 82, 3, None, None)
