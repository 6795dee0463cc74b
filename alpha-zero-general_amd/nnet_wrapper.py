"""NeuralNet plugin surface (NeuralNet.py:14-50, GenericNNetWrapper.py:24-277) on the engine: the object `main.py`,
`pit.py:40-66 create_player` and `Coach.py:29-33` expect from `<game>/NNet.py`:

    nnet = NNetWrapper(game, nn_args)                  # nn_args: dict with learn_rate / lr, dropout, epochs, batch_size,
                                                       #          nn_version, q_weight  (main.py:124-156, pit.py:44)
    nnet.predict(board, valid_actions) -> (pi f32[A] probabilities, v f32[P])          (GenericNNetWrapper.py:94-120)
    nnet.train(examples[, validation_set, save_folder, every])                          (:44-92)
    nnet.evaluate(validation_set) -> loss_pi + loss_v; evaluate_details -> the parts    (:159-177)
    nnet.save_checkpoint(folder, filename, additional_keys)                             (:192-205)
    nnet.load_checkpoint(folder, filename) -> the checkpoint dict (state_dict, full_model, embedded args) or None (:207-221)
    nnet.args, nnet.nnet (the trainable torch module), nnet.requestKnowledgeTransfer

The module is one of azg_amd.train's trainable nets (same parameter names as the reference's, so the reference's .pt files load
with strict=True); inference runs on the engine's one-launch MFMA kernels (azg_amd.nnet.*Hip) with the module's current
weights (BatchNorm folded) -- the reference exports to ONNX-runtime on one CPU core at this point (:232-277).  The evaluator is
rebuilt lazily after every weight change (train / load_checkpoint).  `predict_batch` is the batched form the engine uses."""
import collections
import copy
import os
import pickle
import zlib

import numpy as np
import torch

from . import _lib, nnet as _nn, train as _train

# nn_version -> trainable module per game (splendor/SplendorNNet.py V80, azul/AzulNNet.py V84, santorini/SantoriniNNet.py V89/V78,
# abalone/AbaloneNNet.py V21, smallworld/SmallworldNNet.py V62, akropolis/AkropolisNNet.py V31, minivilles/MinivillesNNet.py V82,
# thelittleprince/TLPNNet.py V83, botanik/BotanikNNet.py V10 / V11)
_DEFAULT_VERSION = {(_lib.SPLENDOR, 2): 80, (_lib.SPLENDOR, 3): 80, (_lib.SPLENDOR, 4): 80, (_lib.AZUL, 2): 84,
                    (_lib.SANTORINI, 1): 89, (_lib.SANTORINI, 11): 78}


def _engine(hip, base, num_players=True):
    """evaluator factory (state_dict, game, device, max_batch) -> hip(base(state_dict[, num_players=P], device=...), max_batch=...)"""
    def make(sd, game, device, max_batch):
        kw = dict(num_players=game.P) if num_players else {}
        return hip(base(sd, device=device, **kw), max_batch=max_batch)
    make.base, make.takes_num_players = base, bool(num_players)        # (read by the tests that evaluate the folded net on its own)
    return make


def _splendor_v80(sd, game, device, max_batch):
    if game.P == 2:
        return _nn.SplendorV80Hip(sd, num_players=2, device=device, max_batch=max_batch)
    return _nn.MobileNet1dHip(_nn.SplendorV80(sd, num_players=game.P, device=device), max_batch=max_batch)


_splendor_v80.base, _splendor_v80.takes_num_players = _nn.SplendorV80, True

EngineNet = collections.namedtuple('EngineNet', 'game variants version module evaluator')
# the engine nets: game id, game variants (None = any), nn_version, trainable module (azg_amd.train) and the factory of its engine-kernel
# evaluator.  (Santorini 88 is a different trunk in the reference, SantoriniNNet.py:167-192: not built)
ENGINE_NETS = (
    EngineNet(_lib.SPLENDOR, None, 80, _train.SplendorV80Module, _splendor_v80),
    EngineNet(_lib.AZUL, None, 84, _train.AzulV84Module, _engine(_nn.MobileNet1dHip, _nn.AzulV84)),
    EngineNet(_lib.SANTORINI, (1,), 89, _train.SantoriniV89Module, _engine(_nn.SantoriniV89Hip, _nn.SantoriniV89, num_players=False)),
    EngineNet(_lib.SANTORINI, (11,), 78, _train.SantoriniV78Module, _engine(_nn.SantoriniV78Hip, _nn.SantoriniV78, num_players=False)),
    EngineNet(_lib.ABALONE, None, 21, _train.AbaloneV21Module, _engine(_nn.AbaloneV21Hip, _nn.AbaloneV21, num_players=False)),
    EngineNet(_lib.SMALLWORLD, None, 62, _train.SmallworldV62Module, _engine(_nn.SmallworldV62Hip, _nn.SmallworldV62)),
    EngineNet(_lib.AKROPOLIS, None, 31, _train.AkropolisV31Module, _engine(_nn.AkropolisV31Hip, _nn.AkropolisV31)),
    EngineNet(_lib.MINIVILLES, None, 82, _train.MinivillesV82Module, _engine(_nn.MobileNet1dHip, _nn.MobileNet1d)),
    EngineNet(_lib.TLP, None, 83, _train.TLPV83Module, _engine(_nn.MobileNet1dHip, _nn.MobileNet1d)),
    EngineNet(_lib.BOTANIK, None, 10, _train.BotanikV10Module, _engine(_nn.BotanikV1xHip, _nn.BotanikV1x, num_players=False)),
    EngineNet(_lib.BOTANIK, None, 11, _train.BotanikV11Module, _engine(_nn.BotanikV1xHip, _nn.BotanikV1x, num_players=False)),
)
_BY_MODULE = {r.module: r for r in ENGINE_NETS}


def _module_for(game, version, dropout):
    for r in ENGINE_NETS:
        if r.game == game.GAME_ID and r.version == version and (r.variants is None or game.variant in r.variants):
            return r.module(game.P, game.A, dropout)
    raise ValueError('nn_version %r is not built for this game (engine nets: %s)' % (version, ', '.join(
        '%s%s' % (r.module.__name__[:-len('Module')], '' if r.variants is None else ' (variant %s)' % '/'.join(map(str, r.variants)))
        for r in ENGINE_NETS)))


def _engine_net(module):
    """the table row of the first class in module's MRO that has one (a subclass of an engine module keeps its engine net), or None"""
    return next((_BY_MODULE[c] for c in type(module).__mro__ if c in _BY_MODULE), None)


def is_engine_module(module):
    return _engine_net(module) is not None


def evaluator_for(module, game, max_batch):
    """engine-kernel evaluator (one launch per leaf batch) of a trainable module's current weights; any other torch module is evaluated
    by PyTorch-ROCm (nnet.TorchModuleEvaluator)"""
    row = _engine_net(module)
    if row is None:
        return _nn.TorchModuleEvaluator(module, game, max_batch)
    sd = {k: v.detach().cpu() for k, v in module.state_dict().items()}
    return row.evaluator(sd, game, str(game.device), max_batch)


def decode_examples(examples):
    """Coach's example list (5-tuples, or zlib-compressed pickles of them, Coach.py:84) -> five stacked arrays"""
    ex = [e if isinstance(e, tuple) else pickle.loads(zlib.decompress(e)) for e in examples]
    return [np.stack([np.asarray(e[k]).reshape(-1) for e in ex]) for k in range(5)]


class NNetWrapper:
    def __init__(self, game, nn_args, module=None):
        """module: a torch module with the reference's forward signature for a game / architecture without an engine net (the f4
        games with the reference's <G>NNet classes); inference then runs it on PyTorch-ROCm (nnet.TorchModuleEvaluator)"""
        self.game = game
        self.args = nn_args
        self.board_size, self.action_size, self.num_players = game.getBoardSize(), game.getActionSize(), game.num_players
        self.requestKnowledgeTransfer = False
        ver = self._arg('nn_version', -1)
        self.nnet, self._custom = module, module is not None
        if module is not None:
            pass
        elif ver is not None and ver > 0:
            self.nnet = _module_for(game, ver, float(self._arg('dropout', 0.0) or 0.0))
        else:
            # pit.py:44 builds the wrapper with nn_version = -1 and lets load_checkpoint bring the model (:258-260)
            dv = _DEFAULT_VERSION.get((game.GAME_ID, game.variant))
            self.nnet = _module_for(game, dv, float(self._arg('dropout', 0.0) or 0.0)) if dv else None
        self._eval, self._eval_batch = None, 0
        self.validation_history = []                    # (step, validation loss) of the last train() with a validation_set

    def _arg(self, k, d=None):
        a = self.args
        v = a.get(k, d) if isinstance(a, dict) else getattr(a, k, d)
        return d if v is None else v

    # ---- inference ----
    def evaluator(self, max_batch=1):
        """the engine-kernel net for leaf batches up to max_batch (what SelfPlayEngine / BatchedMCTS call per round)"""
        if self._eval is None or self._eval_batch < max_batch:
            self._eval, self._eval_batch = evaluator_for(self.nnet, self.game, max_batch), max_batch
        return self._eval

    def predict_batch(self, boards, valids):
        return self.evaluator(int(boards.shape[0])).predict_batch(boards, valids)

    def predict(self, board, valid_actions):
        """NeuralNet.predict (NeuralNet.py:32-43): one board -> (pi probabilities f32[A], v f32[P]) as numpy arrays"""
        dev = self.game.device
        b = torch.from_numpy(np.ascontiguousarray(board, dtype=np.int8)).to(dev).reshape((1,) + tuple(self.board_size))
        m = torch.from_numpy(np.ascontiguousarray(np.asarray(valid_actions).astype(np.uint8))).to(dev).reshape(1, -1)
        pi, v = self.evaluator(1).predict_batch(b, m)
        return pi[0].float().cpu().numpy(), v[0].float().cpu().numpy()

    # ---- training (GenericNNetWrapper.train :44-92) ----
    def train(self, examples, validation_set=None, save_folder=None, every=0, seed=None, log=None):
        """With a validation_set: every `every` steps (when (i_batch + steps_per_epoch * epoch) % every == 0, :86) the set is evaluated
        with the weights and BatchNorm statistics of that moment, the loss goes to `log` (print when None) and into
        self.validation_history as (step, loss), and where i_batch > 0 and save_folder is given intermediary_<i_batch>.pt is saved (:89-90).
        nn_args['device_batches'] (default False): draw, gather and score the batches on the GPU (train.train(device_batches=True))
        nn_args['device_optimizer'] / nn_args['graph_step'] (default False): the one-launch AdamW + OneCycleLR, and a step as one graph
        replay (train.train(device_optimizer=True) / (graph_step=True)); both need device_batches"""
        cols = self._cols(examples)
        on_step = None
        self.validation_history = []
        if validation_set is not None and len(validation_set):
            every = int(every)
            if every < 1:
                raise ValueError('train: a validation_set needs every >= 1 (got %r)' % (every,))
            vcols = self._cols(validation_set)
            say = log or print

            def on_step(epoch, i_batch, step):
                if step % every:
                    return
                self._eval = None                                        # the engine kernel must see the current weights
                loss = self.evaluate(vcols)
                self.validation_history.append((step, loss))
                say('step %d: validation loss %.6f' % (step, loss))
                self.nnet.train()
                if i_batch > 0 and save_folder:
                    self.save_checkpoint(save_folder, filename='intermediary_%d.pt' % i_batch)
        lr = self._arg('learn_rate', self._arg('lr', 3e-3))
        hist = _train.train(self.nnet, cols, learn_rate=float(lr), batch_size=int(self._arg('batch_size', 32)),
                            epochs=int(self._arg('epochs', 1)), q_weight=float(self._arg('q_weight', 0.5)),
                            device=str(self.game.device), seed=seed, log=log, board_shape=self.board_size if self._custom else None,
                            on_step=on_step, device_batches=bool(self._arg('device_batches', False)),
                            device_optimizer=bool(self._arg('device_optimizer', False)), graph_step=bool(self._arg('graph_step', False)))
        self._eval = None
        return hist

    @staticmethod
    def _cols(examples):
        """Coach's example list -> the five stacked arrays; five arrays / tensors pass through"""
        return decode_examples(examples) if isinstance(examples, (list, tuple)) and len(examples) and not hasattr(examples[0], 'shape') \
            else examples

    # ---- validation (GenericNNetWrapper.evaluate :159-177) ----
    def evaluate_details(self, validation_set, batch=4096):
        """dict(loss_pi, loss_v, top1, floored, n) of the net's current weights on validation_set (nnet.evaluate_examples): the forward on
        the engine's one-launch kernel in chunks of `batch`, the losses by azg_eval_losses, one device-to-host read"""
        cols = self._cols(validation_set)
        n = int(cols[0].shape[0])
        return _nn.evaluate_examples(self.evaluator(max(1, min(n, int(batch)))), cols, float(self._arg('q_weight', 0.5)), batch=batch)

    def evaluate(self, validation_set):
        """loss_pi + loss_v as a float -- no 0.25 on the value loss here, exactly as the reference (:176)"""
        d = self.evaluate_details(validation_set)
        return d['loss_pi'] + d['loss_v']

    def loss_pi(self, targets, outputs):
        return _train.loss_pi(targets, outputs)

    def loss_v(self, targets_V, targets_Q, outputs):
        return _train.loss_v(targets_V, targets_Q, outputs, float(self._arg('q_weight', 0.5)))

    # ---- checkpoints (:192-221) ----
    def save_checkpoint(self, folder='checkpoint', filename='checkpoint.pth.tar', additional_keys={}):
        os.makedirs(folder, exist_ok=True)
        cpu = copy.deepcopy(self.nnet).cpu()
        data = {'state_dict': cpu.state_dict(), 'full_model': cpu}
        data.update(additional_keys)
        torch.save(data, os.path.join(folder, filename))

    def load_checkpoint(self, folder='checkpoint', filename='checkpoint.pth.tar'):
        path = os.path.join(folder, filename)
        if not os.path.exists(path):
            print('No model in path {}'.format(path))
            return None
        try:
            ck = torch.load(path, map_location='cpu', weights_only=False)
        except Exception:
            # a reference checkpoint pickles its own module class as `full_model`; without the reference's package on
            # sys.path only the tensors and the embedded args can be read
            ck = _load_without_full_model(path)
            if ck is None:
                print("MODEL {} CAN'T BE READ but file exists".format(path))
                return None
        ver = getattr(ck.get('full_model'), 'version', ck.get('nn_version'))
        want = self._arg('nn_version', -1)
        if not self._custom and want is not None and want > 0 and ver is not None and ver != want:          # :250-253
            print('Checkpoint includes NN version', ver, ', but you ask version', want, ' so not loading it and initiate knowledge transfer')
            self.requestKnowledgeTransfer = True
            return ck
        try:
            # the replacement module is built and filled in a local: self.nnet changes only when the whole load succeeded (the
            # reference's load_network keeps its existing net when the state dict does not fit, GenericNNetWrapper.py:262-267)
            target = self.nnet
            if not self._custom and (target is None or getattr(target, 'version', None) != ver):
                target = _module_for(self.game, ver, float(self._arg('dropout', 0.0) or 0.0))
            sd = {k: torch.as_tensor(np.asarray(v)) if not torch.is_tensor(v) else v for k, v in ck['state_dict'].items()}
            if target is self.nnet and target is not None:
                # load_state_dict copies tensor by tensor: check the fit first, so that a mismatch cannot leave a half-loaded net
                own = target.state_dict()
                bad = [k for k in own if k not in sd or tuple(sd[k].shape) != tuple(own[k].shape)] + [k for k in sd if k not in own]
                if bad:
                    raise RuntimeError('state dict does not fit: %s' % ', '.join(bad[:4]))
            target.load_state_dict(sd, strict=True)
        except (RuntimeError, ValueError) as ex:                         # another architecture: GenericNNetWrapper.py:262-267
            print('Could not load state dict (%s), initiate knowledge transfer' % str(ex).splitlines()[0])
            self.requestKnowledgeTransfer = True
            self._eval = None                                            # (nothing cached may outlive a failed load)
            return ck
        self.nnet = target
        self._eval = None
        return ck


class _Opaque:
    """placeholder for a pickled object whose class cannot be imported (the reference's `full_model`)"""

    def __init__(self, *a, **k):
        pass

    def __setstate__(self, state):
        self.__dict__['_state'] = state


def _load_without_full_model(path):
    import pickle as _p

    class U(_p.Unpickler):
        def find_class(self, module, name):
            try:
                return super().find_class(module, name)
            except Exception:
                return _Opaque

    class P:                                            # the `pickle_module` interface torch.load expects
        Unpickler = U
        load = staticmethod(_p.load)
        __name__ = 'pickle'

    try:
        ck = torch.load(path, map_location='cpu', weights_only=False, pickle_module=P)
    except Exception:
        return None
    fm = ck.get('full_model')
    if isinstance(fm, _Opaque):
        ck['full_model'] = None
    return ck
