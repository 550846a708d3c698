"""The model of evaluation (tests/evalref.py) against torch.nn.BatchNorm2d -- momentum, track_running_stats, .eval() -- so that the
yardstick of tests/test_gpu_eval.py is pinned by something that is not this project; its order and plan helpers against the library's
host-only functions; and the refusals that need no device.  (Every mi_trainer_* refusal needs a trainer, and init_trainer a device:
those are in tests/test_gpu_eval.py.  mi_op_bn_running_update checks its arguments before any device call and is reached here.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import evalref as E
import synth
import torch_ref as T

# (N, C, H): one sample per channel pair (n = 2), a single channel, an odd plane, a wide layer
SHAPES = [(2, 3, 1), (4, 1, 3), (3, 5, 7), (2, 64, 4)]


def _tensors(shape, steps, seed):
    N, Cc, H = shape
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(N, Cc, H, H, generator=g, dtype=torch.float64) * (1 + s) + 0.5 * s for s in range(steps)]


@pytest.mark.parametrize("momentum", [0.1, 0.5, 1.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_update_rule_and_eval_output_are_batchnorm2d(shape, momentum):
    N, Cc, H = shape
    eps = 1e-5
    bn = torch.nn.BatchNorm2d(Cc, eps=eps, momentum=momentum, dtype=torch.float64)
    with torch.no_grad():
        bn.weight.copy_(torch.linspace(0.5, 1.5, Cc, dtype=torch.float64))
        bn.bias.copy_(torch.linspace(-0.2, 0.3, Cc, dtype=torch.float64))
    state = E.new_state(Cc)
    assert torch.equal(state["mean"], bn.running_mean) and torch.equal(state["var"], bn.running_var)
    bn.train()
    for x in _tensors(shape, 3, 7):
        want = bn(x)
        got = E.bn_track(x, bn.weight, bn.bias, eps, state, momentum)
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
        assert torch.allclose(got, T.bn_train(x, bn.weight, bn.bias, eps), rtol=1e-12, atol=1e-12)  # training output: TorchNet's own
        assert torch.allclose(state["mean"], bn.running_mean, rtol=1e-12, atol=1e-14)
        assert torch.allclose(state["var"], bn.running_var, rtol=1e-12, atol=1e-14)
    assert state["updates"] == int(bn.num_batches_tracked) == 3
    bn.eval()
    x = _tensors(shape, 4, 11)[3]
    before = (state["mean"].clone(), state["var"].clone())
    assert torch.allclose(E.bn_eval(x, bn.weight, bn.bias, eps, state), bn(x), rtol=1e-12, atol=1e-12)
    assert torch.equal(before[0], state["mean"]) and torch.equal(before[1], state["var"]) and int(bn.num_batches_tracked) == 3


def test_momentum_one_keeps_the_batch_statistics():
    x = _tensors((3, 5, 7), 1, 3)[0]
    state = E.new_state(5)
    E.bn_track(x, torch.ones(5, dtype=torch.float64), torch.zeros(5, dtype=torch.float64), 1e-5, state, 1.0)
    assert torch.equal(state["mean"], x.mean(dim=(0, 2, 3)))
    n = 3 * 49
    assert torch.allclose(state["var"], x.var(dim=(0, 2, 3), unbiased=True), rtol=1e-13)
    assert abs(float(E.unbias(n)) - n / (n - 1)) <= 2.0 ** -24 * n / (n - 1)


def test_without_tracking_batchnorm2d_is_the_training_forward():
    """track_running_stats=False: the module has no running statistics and normalises with the batch's in .eval() too -- what
    forward_pass does, and what TorchNet models"""
    x = _tensors((3, 5, 7), 1, 5)[0]
    bn = torch.nn.BatchNorm2d(5, eps=1e-5, track_running_stats=False, dtype=torch.float64)
    assert bn.running_mean is None and bn.running_var is None
    bn.eval()
    assert torch.allclose(bn(x), T.bn_train(x, bn.weight, bn.bias, 1e-5), rtol=1e-12, atol=1e-12)


def test_unbias_is_the_librarys():
    from resnet_amd import binding as B
    L = B.load()
    for n in (-3, 0, 1):
        assert L.mi_bn_unbias(n) == 1.0 and E.unbias(n) == 1.0
    # per-layer counts of the networks under test, and the same with a world factor of 8 (sync-BN: n = batch x plane x world)
    for n in (2, 3, 98, 4 * 16 * 16, 256 * 112 * 112, 8 * 256 * 112 * 112, 2 ** 40 + 1):
        got = np.float32(L.mi_bn_unbias(n))
        assert got.tobytes() == E.unbias(n).tobytes(), n
        assert got == np.float32(np.float64(n) / np.float64(n - 1))


@pytest.mark.parametrize("name", ["C1", "C1S", "C4I", "R50"])
def test_layer_order_follows_the_gammas_of_locations(name):
    dims = getattr(synth, name + "_DIMS")
    gammas = [size for size, kind, _ in synth.location_table(dims) if kind == "g"]
    assert E.bn_channels(dims) == gammas
    assert len(E.bn_planes(dims)) == len(E.bn_names(dims)) == len(gammas)
    if name == "R50":
        assert len(gammas) == 53 and sum(gammas) == 26560
        assert E.bn_planes(dims)[:5] == [112, 56, 56, 56, 56] and E.bn_planes(dims)[-1] == 7
        assert E.bn_names(dims)[4] == "batch_norms/00/projected/" and E.bn_names(dims)[5] == "batch_norms/01/reduced/"


def test_center_plan_is_mi_augment_plan():
    from resnet_amd import binding as B
    L = B.load()
    for n, dim_in, dim_out in [(5, 40, 32), (3, 41, 32), (1, 32, 32), (7, 256, 224)]:
        out = np.full((n, 3), -1, np.int32)
        assert L.mi_augment_plan(B.MI_AUG_CENTER, 0, 0, 0, 12345, n, dim_in, dim_out, None, out.ctypes.data) == 0
        assert np.array_equal(out, E.center_plan(n, dim_in, dim_out))


def test_eval_net_tracks_without_changing_the_training_forward():
    dims, batch = synth.C1_DIMS, 3
    params = synth.make_params(dims, perturb_bn=True)
    im, lab = synth.make_batch(dims, batch)
    x = T.nhwc_to_nchw(im)
    plain, net = T.TorchNet(dims, params), E.EvalNet(dims, params, momentum=1.0)
    assert float(plain.forward(x, lab).detach()) == float(net.forward(x, lab).detach())
    means, vars_ = net.running()
    assert means.size == vars_.size == sum(E.bn_channels(dims))
    y = net.acts["stem_conv"].detach()
    assert np.array_equal(means[:64], y.mean(dim=(0, 2, 3)).numpy())
    assert [s["updates"] for s in net.state] == [1] * 5
    # eval with the statistics of this very batch is NOT the training forward (unbiased variance), but is close to it; and it
    # leaves the state alone
    logits = net.eval_forward(x)
    assert np.array_equal(net.running()[0], means) and [s["updates"] for s in net.state] == [1] * 5
    assert logits.shape == (batch, dims["output"]) and np.all(np.isfinite(logits))
    assert not np.array_equal(logits, plain.acts["logits"].detach().numpy())
    # rows do not see each other in eval: the first row alone gives the first row's logits
    alone = net.eval_forward(np.concatenate([x[:1], np.zeros_like(x[1:])]))
    assert np.allclose(alone[0], logits[0], rtol=1e-10, atol=1e-12)


def _layer_arrays(n=1, ch=4):
    return ((C.c_void_p * n)(*([1] * n)), (C.c_void_p * n)(*([1] * n)), (C.c_int * n)(*([ch] * n)), (C.c_int64 * n)(*([2] * n)))


@pytest.mark.parametrize("momentum", [0.0, 1.5, -0.1, float("nan")])
def test_running_update_refuses_a_momentum_outside_0_1(momentum):
    from resnet_amd import binding as B
    L = B.load()
    L.mi_clear_error()
    pm, pv, ch, cnt = _layer_arrays()
    try:
        assert L.mi_op_bn_running_update(pm, pv, ch, cnt, 1, C.c_void_p(1), 4, momentum) == -1  # (no pointer is followed: refused first)
        assert b"momentum lies in (0, 1]" in L.mi_last_error()
    finally:
        L.mi_clear_error()


def test_running_update_refuses_bad_tables():
    from resnet_amd import binding as B
    L = B.load()
    pm, pv, ch, cnt = _layer_arrays()
    cases = [((pm, pv, ch, cnt, 0, C.c_void_p(1), 4, 0.1), b"at least one layer"),
             ((pm, pv, ch, cnt, 1, None, 4, 0.1), b"no NULL array"),
             ((pm, pv, ch, cnt, 1, C.c_void_p(1), 3, 0.1), b"exceed running_channels"),
             ((pm, pv, (C.c_int * 1)(0), cnt, 1, C.c_void_p(1), 4, 0.1), b"at least one channel"),
             ((pm, pv, ch, (C.c_int64 * 1)(0), 1, C.c_void_p(1), 4, 0.1), b"count is at least 1"),
             (((C.c_void_p * 1)(None), pv, ch, cnt, 1, C.c_void_p(1), 4, 0.1), b"both statistics")]
    for args, word in cases:
        L.mi_clear_error()
        try:
            assert L.mi_op_bn_running_update(*args) == -1
            assert word in L.mi_last_error(), (word, L.mi_last_error())
        finally:
            L.mi_clear_error()
