"""CPU: the float64 model of momentum SGD and LARS (optim_ref.py) that the GPU tests hold the kernels to, and the operator's
refusals that happen before any device work."""
import ctypes as C

import numpy as np
import pytest

import optim_ref as R


def test_sgd_model_matches_torch_optim_sgd_over_5_steps():
    import torch
    rng = np.random.default_rng(5)
    shapes = [(64, 3, 7, 7), (64,), (64,), (1000, 2048 // 16)]
    ws = [rng.standard_normal(s) * 10.0 ** rng.uniform(-3, 1) for s in shapes]
    params = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in ws]
    opt = torch.optim.SGD(params, lr=0.05, momentum=0.9, dampening=0, nesterov=False, weight_decay=5e-5)
    mine_w, mine_b = [w.ravel() for w in ws], [np.zeros(w.size) for w in ws]
    for _ in range(5):
        gs = [rng.standard_normal(s) * 10.0 ** rng.uniform(-3, 1) for s in shapes]
        for p, g in zip(params, gs):
            p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        mine_w, out_g, mine_b, flag = R.step(R.SGD, mine_w, gs, mine_b, [1] * len(shapes), 0.05, 5e-5, 0.9)
        assert flag == 0 and not any(np.any(g) for g in out_g)
        for p, w, b in zip(params, mine_w, mine_b):
            ref_w = p.detach().numpy().ravel()
            ref_b = opt.state[p]["momentum_buffer"].numpy().ravel()
            assert np.max(np.abs(w - ref_w)) <= 1e-12 * max(1.0, np.max(np.abs(ref_w)))
            assert np.max(np.abs(b - ref_b)) <= 1e-12 * max(1.0, np.max(np.abs(ref_b)))


def test_lars_model_on_a_hand_worked_example():
    """lr 0.1, wd 0.1, mu 0.9, tau 0.01.
    weight A: w (3, 4), g (0.3, 0.4): |w| 5, |g| 0.5, trust 0.01 * 5 / (0.5 + 0.1 * 5) = 0.05; g + wd w = (0.6, 0.8);
              b (1, -1) -> 0.9 b + 0.1 * 0.05 * (0.6, 0.8) = (0.903, -0.896);  w -> (2.097, 4.896)
    weight Z: w (0, 0) has zero norm: trust 1;  b (0, 0.5) -> 0.9 b + 0.1 * (0.3 + 0, -0.4 + 0) = (0.03, 0.41);  w -> (-0.03, -0.41)
    BN beta: no trust, no weight decay: w (2, 0), g (1, -2), b (0.5, 0) -> 0.9 b + 0.1 g = (0.55, -0.2);  w -> (1.45, 0.2)"""
    ws = [np.array([3.0, 4.0]), np.array([0.0, 0.0]), np.array([2.0, 0.0])]
    gs = [np.array([0.3, 0.4]), np.array([0.3, -0.4]), np.array([1.0, -2.0])]
    bs = [np.array([1.0, -1.0]), np.array([0.0, 0.5]), np.array([0.5, 0.0])]
    assert R.trust_ratio(25.0, 0.25, 0.1, 0.01) == pytest.approx(0.05, rel=1e-15)
    w, g, b, flag = R.step(R.LARS, ws, gs, bs, [1, 1, 0], lr=0.1, wd=0.1, momentum=0.9, tau=0.01)
    assert flag == 0
    np.testing.assert_allclose(b[0], [0.903, -0.896], rtol=0, atol=1e-15)
    np.testing.assert_allclose(w[0], [2.097, 4.896], rtol=0, atol=1e-14)
    np.testing.assert_allclose(b[1], [0.03, 0.41], rtol=0, atol=1e-15)
    np.testing.assert_allclose(w[1], [-0.03, -0.41], rtol=0, atol=1e-15)
    np.testing.assert_allclose(b[2], [0.55, -0.2], rtol=0, atol=1e-15)
    np.testing.assert_allclose(w[2], [1.45, 0.2], rtol=0, atol=1e-15)
    assert not any(np.any(x) for x in g)


@pytest.mark.parametrize("kind", [R.SGD, R.LARS])
def test_model_guards(kind):
    """NaN in tensor 3, Inf in tensor 1: the flag names 3; their non-finite gradients stay, every other gradient is cleared; LARS
    keeps those whole tensors, SGD the offending elements"""
    rng = np.random.default_rng(1)
    ws = [rng.standard_normal(8) for _ in range(5)]
    gs = [rng.standard_normal(8) for _ in range(5)]
    bs = [rng.standard_normal(8) for _ in range(5)]
    gs[3][2], gs[1][5] = np.nan, np.inf
    w, g, b, flag = R.step(kind, ws, gs, bs, [1, 0, 1, 1, 0], 0.1, 5e-5, 0.9)
    assert flag == 4
    for i in range(5):
        bad = {1: 5, 3: 2}.get(i)
        if bad is None:
            assert not np.any(g[i]) and np.all(w[i] != ws[i]) and np.all(b[i] != bs[i])
            continue
        assert not np.isfinite(g[i][bad]) and np.count_nonzero(g[i]) == 1
        if kind == R.LARS:
            assert np.array_equal(w[i], ws[i]) and np.array_equal(b[i], bs[i])
        else:
            assert w[i][bad] == ws[i][bad] and b[i][bad] == bs[i][bad]
            others = np.arange(8) != bad
            assert np.all(w[i][others] != ws[i][others])


def test_momentum_update_operator_refuses_bad_arguments_before_any_device_work():
    """kind Adam, offsets off the 16-byte grid, tensors beyond n: -1 with mi_last_error set (host-side checks: no GPU needed)"""
    from resnet_amd import binding as B
    L = B.load()
    off = (C.c_size_t * 3)(0, 64, 128)
    isw = (C.c_int * 2)(1, 0)
    cases = [(B.MI_OPT_ADAM, off, 128), (B.MI_OPT_LARS, off, 100), (B.MI_OPT_SGD, (C.c_size_t * 3)(0, 62, 128), 128)]
    for kind, o, n in cases:
        L.mi_clear_error()
        assert L.mi_op_momentum_update(kind, None, None, None, n, o, 2, isw, 0.1, 0.0, 0.9, 0.001, None, None) == -1
        assert L.mi_last_error().decode()
    L.mi_clear_error()
