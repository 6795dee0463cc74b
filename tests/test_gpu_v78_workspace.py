"""The raw-logits workspace of the with-gods net's two-launch policy FC (k_s78_policy_gemm_h2 -> k_s78_policy_softmax) belongs to the net
object: every SantoriniV78Hip -- a clone_buffers() copy included -- has its own, so forwards on concurrent streams and a forward captured
into a graph cannot meet in it."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
W = os.path.join(os.path.dirname(__file__), 'golden', 'weights_santorini11_v78.npz')


@pytest.fixture(scope='module')
def base():
    from azg_amd import nnet
    return nnet.SantoriniV78.from_npz(W, device='cuda:0')


def _inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    boards = torch.randint(-2, 5, (B, 75), generator=g, dtype=torch.int8).to('cuda:0')
    valid = (torch.rand((B, 1782), generator=g) < 0.05).to(torch.uint8)
    valid[:, 7] = 1
    return boards, valid.to('cuda:0')


def _alone(net, boards, valid):
    pi, v = net.predict_batch(boards, valid)
    torch.cuda.synchronize()
    return pi.clone(), v.clone()


def test_every_net_object_owns_its_workspace(base):
    from azg_amd import nnet
    net = nnet.SantoriniV78Hip(base, max_batch=64)
    other = net.clone_buffers()
    assert net.logits.shape == (64, 1792) and other.logits.shape == (64, 1792)
    assert other.logits.data_ptr() != net.logits.data_ptr()
    assert other.pi.data_ptr() != net.pi.data_ptr() and other._keep is net._keep
    boards, valid = _inputs(65, 1)
    net.predict_batch(boards, valid)                   # B > max_batch: the buffers grow, the workspace with them
    torch.cuda.synchronize()
    assert net.maxB >= 65 and net.logits.shape[0] >= 65 and net.logits.shape[1] == 1792
    assert other.logits.shape[0] == 64


@pytest.mark.parametrize('B', [65, 203])                # the second 64-sample GEMM row group holds one sample / ragged in the GEMM and the softmax
def test_a_net_and_its_clone_on_two_streams(base, B):
    from azg_amd import nnet
    net = nnet.SantoriniV78Hip(base, max_batch=256)
    other = net.clone_buffers()
    in_a, in_b = _inputs(B, 10 + B), _inputs(B, 20 + B)
    assert not torch.equal(in_a[0], in_b[0])
    ref_a, ref_b = _alone(net, *in_a), _alone(other, *in_b)
    assert not torch.equal(ref_a[0], ref_b[0])
    for t in (net.pi, net.v, net.logits, other.pi, other.v, other.logits):
        t.zero_()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    for _ in range(4):                                 # issued back to back, nothing synchronises the two streams
        with torch.cuda.stream(s1):
            pa, va = net.predict_batch(*in_a)
        with torch.cuda.stream(s2):
            pb, vb = other.predict_batch(*in_b)
    torch.cuda.synchronize()
    assert torch.equal(pa, ref_a[0]) and torch.equal(va, ref_a[1])
    assert torch.equal(pb, ref_b[0]) and torch.equal(vb, ref_b[1])


def test_a_captured_forward_survives_a_larger_batch_of_another_net(base):
    from azg_amd import nnet
    net = nnet.SantoriniV78Hip(base, max_batch=64)
    boards, valid = _inputs(64, 3)
    ref = _alone(net, boards, valid)                   # (also the warm-up: every kernel has run before the capture)
    net.pi.zero_()
    net.v.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net.predict_batch(boards, valid)               # three kernel nodes in a row: a single branch
    second = nnet.SantoriniV78Hip(base, max_batch=64)
    big = _inputs(203, 4)
    second.predict_batch(*big)                         # grows the second net's buffers
    torch.cuda.synchronize()
    assert second.logits.shape[0] >= 203 and net.logits.shape[0] == 64
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(net.pi[:64], ref[0]) and torch.equal(net.v[:64], ref[1])


def test_one_launch_form_has_no_workspace(base):
    from azg_amd import nnet
    net = nnet.SantoriniV78Hip(base, max_batch=64, policy2=False)
    assert not hasattr(net, 'logits') and not hasattr(net.clone_buffers(), 'logits')
    ref = nnet.SantoriniV78.from_npz(W, device='cuda:0', dtype=torch.float64)
    boards, valid = _inputs(203, 5)
    rm = valid.bool()
    pi, v = net.predict_batch(boards, valid)
    pr, vr = ref.predict_batch(boards.reshape(203, 5, 5, 3), rm)
    assert float((pi - pr).abs().max()) < 1e-5 and float((v - vr).abs().max()) < 1e-5
    assert float(pi[~rm].abs().max()) == 0.0
