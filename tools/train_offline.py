#!/usr/bin/env python3
"""The reference's offline trainer (GenericNNetWrapper.py:347-441, `python GenericNNetWrapper.py <game> ...`) on the engine: retrain a net,
or try another nn_version, on a stored `checkpoint.examples` without playing a game.
    python tools/train_offline.py splendor -i nets/best.pt                       print the net and the checkpoint's embedded keys
    python tools/train_offline.py splendor -i nets/best.pt -T checkpoint.examples -o retrained_ -b 512
    python tools/train_offline.py splendor -V 80 -T checkpoint.examples -t other.examples
With --training: the example history is flattened, the last tenth is held out as the test set unless --test names a file, the last
nb_samples * 1000 of the rest are trained on with the test set validated every 1e5 // batch_size - 1 steps (NNetWrapper.train: the forward
of the validation on the engine's one-launch kernel, the losses by azg_eval_losses), intermediary_<i>.pt and at the end last.pt are written
into <output><last six digits of the time>/.  Same flags and defaults as the reference; no FLOP count is printed (that needs fvcore).
--device-batches (not in the reference): the training batches are drawn, gathered and scored on the GPU, nothing is read back per step.
--device-optimizer / --graph-step (not in the reference; both need --device-batches): AdamW + OneCycleLR in one launch with the step number
on the GPU / a whole training step as one replay of a captured graph."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# games whose constructor takes the number of players / a variant (azg_amd.games)
_NUM_PLAYERS = ('splendor', 'minivilles', 'thelittleprince', 'akropolis', 'smallworld')


def build_parser():
    parser = argparse.ArgumentParser(description='NNet loader')
    parser.add_argument('game', action='store', default='splendor', help='The name of the game to play')
    parser.add_argument('--input', '-i', action='store', default=None, help='Input NN to load')
    parser.add_argument('--output', '-o', action='store', default=None, help='Prefix for output NN')
    parser.add_argument('--training', '-T', action='store', default=None, help='checkpoint.examples file to train on')
    parser.add_argument('--test', '-t', action='store', default=None, help='checkpoint.examples file to validate on (default: the last tenth of --training)')

    parser.add_argument('--learn-rate', '-l', action='store', default=0.0003, type=float, help='')
    parser.add_argument('--dropout', '-d', action='store', default=0.3, type=float, help='')
    parser.add_argument('--epochs', '-p', action='store', default=2, type=int, help='')
    parser.add_argument('--batch-size', '-b', action='store', default=32, type=int, help='')
    parser.add_argument('--nb-samples', '-N', action='store', default=9999, type=int, help='How many samples (in thousands)')
    parser.add_argument('--nn-version', '-V', action='store', default=-1, type=int, help='Which architecture to choose')
    parser.add_argument('--q-weight', '-q', action='store', default=0.5, type=float, help='Weight for mixing Q into value loss')
    # not in the reference, where a game's module constants say this
    parser.add_argument('--num-players', action='store', default=None, type=int, help='Players (splendor, minivilles, thelittleprince, akropolis, smallworld)')
    parser.add_argument('--variant', action='store', default=None, type=int, help='Santorini: number of gods (1 = no gods, 11); Abalone: the variant word of include/azg.h (1 Belgian Daisy, 2 German Daisy, 3 classic, + 4 dynamic komi)')
    return parser


def add_engine_options(parser):
    """options of the engine's trainer that are no flag of the reference's (build_parser keeps to those)"""
    parser.add_argument('--device-batches', action='store_true', help='Draw, gather and score the training batches on the GPU (train.train(device_batches=True)): no host synchronisation per step')
    parser.add_argument('--device-optimizer', action='store_true', help='AdamW + OneCycleLR as one launch that takes the step number from device memory (train.train(device_optimizer=True)); needs --device-batches')
    parser.add_argument('--graph-step', action='store_true', help='Capture one training step as a graph and replay it for every later step (train.train(graph_step=True)); implies --device-optimizer, needs --device-batches')
    return parser


def make_game(args):
    from azg_amd import games
    kw = {}
    if args.num_players is not None:
        if args.game not in _NUM_PLAYERS:
            raise SystemExit('--num-players: %s has a fixed number of players' % args.game)
        kw['num_players'] = args.num_players
    if args.variant is not None:
        if args.game == 'abalone':
            if not 1 <= args.variant <= 7 or args.variant & 3 == 0:
                raise SystemExit('--variant: abalone takes 1 / 2 / 3 (Belgian Daisy / German Daisy / classic), + 4 for dynamic komi')
            kw.update(layout={1: 'belgian', 2: 'german', 3: 'classic'}[args.variant & 3], dynamic_komi=bool(args.variant & 4))
        elif args.game != 'santorini':
            raise SystemExit('--variant is for santorini and abalone')
        else:
            kw['nb_gods'] = args.variant
    return games.import_game(args.game, **kw)


def flatten(path):
    from azg_amd import formats
    return [e for it in formats.load_train_examples(path) for e in it]


def main(argv=None):
    args = add_engine_options(build_parser()).parse_args(argv)
    sys.path.insert(0, ROOT)
    import torch
    from azg_amd.nnet_wrapper import NNetWrapper

    output = (args.output if args.output else 'output_') + str(int(time.time()))[-6:]
    g = make_game(args)
    nn_args = dict(lr=args.learn_rate, dropout=args.dropout, epochs=args.epochs, batch_size=args.batch_size, nn_version=args.nn_version,
                   learn_rate=args.learn_rate, no_compression=False, q_weight=args.q_weight, device_batches=args.device_batches,
                   device_optimizer=args.device_optimizer, graph_step=args.graph_step)
    nnet = NNetWrapper(g, nn_args)
    if args.input:
        nnet.load_checkpoint(os.path.dirname(args.input), os.path.basename(args.input))
    elif args.nn_version == -1:
        raise Exception('You have to specify at least a NN file to load or a NN version')
    if nnet.nnet is None:
        raise SystemExit('no net: this game has no default nn_version, give --nn-version or --input')
    print('V%s -> nb params %.2e' % (getattr(nnet.nnet, 'version', '?'), sum(p.numel() for p in nnet.nnet.parameters())))

    if not args.training:
        if args.input:
            checkpoint = torch.load(args.input, map_location='cpu', weights_only=False)
            for k in sorted(checkpoint.keys()):
                if k not in ['state_dict', 'full_model', 'optim_state']:
                    print('  %s: %s' % (k, checkpoint[k]))
            print('Board shape: %s, valids shape: %s' % ([1] + list(g.getBoardSize()), [1, g.getActionSize()]))
        return 0

    trainExamples = flatten(args.training)
    if args.test is None:
        splitNumber = len(trainExamples) // 10
        testExamples, trainExamples = trainExamples[-splitNumber:], trainExamples[:-splitNumber]
    else:
        testExamples = flatten(args.test)
    trainExamples = trainExamples[-args.nb_samples * 1000:]
    print('Number of samples: training %d, testing %d; number of epochs %d' % (len(trainExamples), len(testExamples), args.epochs))

    save_every = (1e5 // args.batch_size) - 1
    nnet.train(trainExamples, testExamples, output, save_every)
    nnet.save_checkpoint(output, filename='last.pt')
    print('saved', os.path.join(output, 'last.pt'))
    return 0


if __name__ == '__main__':
    sys.exit(main())
