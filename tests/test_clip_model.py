"""CPU: the model of gradient clipping and of SGD with two decay groups (clipref.py) against torch, the documented departure for a
gradient that is not finite, the sensitivity of the GPU operator test's inputs to the three restated faults, and the operators' refusals
that happen before any device work."""
import ctypes as C

import numpy as np
import pytest

import clipref as M
import optim_ref as R

NEW_SYMBOLS = ["mi_op_clip_grad_norm", "mi_trainer_set_clip_grad_norm", "mi_trainer_last_clip", "mi_trainer_set_norm_weight_decay",
               "mi_op_momentum_update2"]


def test_the_library_exports_the_new_entry_points():
    from resnet_amd import binding as B
    L = B.load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert C.sizeof(B.MiClipRecord) == 40


def _torch_clip(gs, max_norm):
    import torch
    params = [torch.zeros(g.size, dtype=torch.float64, requires_grad=True) for g in gs]
    for p, g in zip(params, gs):
        p.grad = torch.tensor(np.asarray(g, np.float64))
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    return float(total), [p.grad.numpy() for p in params]


@pytest.mark.parametrize("factor", [0.5, 0.999, 2.0], ids=["half", "just-below", "twice"])
def test_model_matches_torch_clip_grad_norm(factor):
    """float64 copies of float32 gradients: the total norm to 1e-12 relative, the scaled gradients to 2^-23 relative (the coefficient's one
    rounding to float32 and the float32 product: half an ulp each)"""
    rng = np.random.default_rng(3)
    gs = [rng.standard_normal(n, dtype=np.float32) * np.float32(10.0 ** rng.uniform(-4, 2)) for n in (64, 4096, 3 * M.CHUNK + 7, 1203)]
    norm = float(np.sqrt(sum(np.sum(g.astype(np.float64) ** 2) for g in gs)))
    max_norm = float(np.float32(factor * norm))
    got, rec = M.clip(gs, max_norm)
    total, want = _torch_clip(gs, max_norm)
    assert abs(rec["norm"] - total) <= 1e-12 * total
    assert abs(rec["sq_norm"] - total * total) <= 4e-12 * total * total
    assert rec["clipped"] == (factor < 1) and rec["nonfinite"] == 0
    for g, a, b in zip(gs, got, want):
        assert a.dtype == np.float32
        assert np.all(np.abs(a.astype(np.float64) - b) <= 2.0 ** -23 * np.abs(b))
        if factor > 1:
            assert np.array_equal(a.view(np.uint32), g.view(np.uint32))


def test_chunk_sums_add_up_and_never_cross_a_tensor():
    gs = M.split(M.op_gradient(), M.OP_OFFSETS)
    part = M.chunk_sq(gs)
    assert part.size == sum(len(R.chunks_of(n)) for n in M.OP_SIZES) == 71
    per_tensor = R.sq_norms(gs, gs)[:, 1]
    at = 0
    for n, want in zip(M.OP_SIZES, per_tensor):
        k = len(R.chunks_of(n))
        assert abs(part[at:at + k].sum() - want) <= 1e-14 * want
        at += k


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_a_gradient_that_is_not_finite_is_left_alone_where_torch_spreads_nan(bad):
    """the documented departure: coef 1, nonfinite 1, every word of the gradient as it was; torch turns the finite gradients into NaN"""
    rng = np.random.default_rng(4)
    gs = [rng.standard_normal(100, dtype=np.float32) for _ in range(3)]
    gs[1][17] = bad
    got, rec = M.clip(gs, 0.5)
    assert rec["coef"] == 1 and rec["nonfinite"] == 1 and rec["clipped"] == 0 and not np.isfinite(rec["sq_norm"])
    for g, a in zip(gs, got):
        assert np.array_equal(a.view(np.uint32), g.view(np.uint32))
    _, want = _torch_clip(gs, 0.5)  # torch: an Inf gives coef 0 (and 0 x Inf = NaN in its place), a NaN gives coef NaN
    assert not np.any(np.isfinite(want[0]) & (want[0] != 0)) and np.isnan(want[1][17])


def test_zero_and_huge_gradients():
    """all zero: coef 1 (max_norm / 1e-6 is clamped); elements near 1e30: the squares overflow float32 but not float64"""
    got, rec = M.clip([np.zeros(100, np.float32)], 1.0)
    assert rec["coef"] == 1 and rec["norm"] == 0 and rec["nonfinite"] == 0 and not np.any(got[0])
    g = np.full(1000, 1e30, np.float32)
    with np.errstate(over="ignore"):
        assert np.isinf(np.sum(g * g))
    got, rec = M.clip([g], 1e30)
    want = 1e30 / np.sqrt(1000.0 * float(g[0]) ** 2)
    assert rec["nonfinite"] == 0 and 0 < rec["coef"] < 1 and abs(float(rec["coef"]) - want) <= 2.0 ** -23 * want


@pytest.mark.parametrize("fault", M.FAULTS)
def test_each_restated_fault_shows_on_the_operator_tests_inputs(fault):
    """test_gpu_clip.py's operator case (a) asks for sq_norm to OP_SQ_REL, coef to one float32 ulp and every element bit for bit: each fault
    must move one of them by more than that on that test's own gradient, at that test's max_norm"""
    g = M.op_gradient()
    gs = M.split(g, M.OP_OFFSETS)
    _, clean = M.clip(gs, 1.0)
    max_norm = float(np.float32(0.5 * clean["norm"]))
    good, rec = M.clip(gs, max_norm)
    assert rec["clipped"] == 1
    bad, frec = M.clip(gs, max_norm, fault)
    if fault == "scale_tail_unscaled":
        assert frec["coef"] == rec["coef"]
        diff = sum(int(np.sum(a.view(np.uint32) != b.view(np.uint32))) for a, b in zip(good, bad))
        assert diff == 3, "the three scalars behind the last float4 of the last tensor"
    else:
        assert abs(frec["sq_norm"] - rec["sq_norm"]) > 1e4 * M.OP_SQ_REL * rec["sq_norm"]
        assert M.ulps32(frec["coef"], rec["coef"]) > 1


def test_two_group_sgd_model_matches_torch_optim_sgd_over_3_steps():
    import torch
    rng = np.random.default_rng(6)
    shapes = [(64, 3, 7, 7), (64,), (64,), (100, 128)]
    is_w = [1, 0, 0, 1]
    wd, wd_norm = 5e-5, 1e-3
    ws = [rng.standard_normal(s) * 10.0 ** rng.uniform(-2, 1) for s in shapes]
    params = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in ws]
    opt = torch.optim.SGD([{"params": [p for p, f in zip(params, is_w) if f], "weight_decay": wd},
                           {"params": [p for p, f in zip(params, is_w) if not f], "weight_decay": wd_norm}],
                          lr=0.05, momentum=0.9, dampening=0, nesterov=False)
    mine_w, mine_b = [w.ravel() for w in ws], [np.zeros(w.size) for w in ws]
    for _ in range(3):
        gs = [rng.standard_normal(s) * 10.0 ** rng.uniform(-2, 1) for s in shapes]
        for p, g in zip(params, gs):
            p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        one_w = R.step(R.SGD, mine_w, gs, mine_b, is_w, 0.05, wd, 0.9)[0]
        mine_w, out_g, mine_b, flag = M.sgd_two_groups(mine_w, gs, mine_b, is_w, 0.05, wd, wd_norm, 0.9)
        assert flag == 0 and not any(np.any(g) for g in out_g)
        for i, (p, w, b) in enumerate(zip(params, mine_w, mine_b)):
            ref_w = p.detach().numpy().ravel()
            ref_b = opt.state[p]["momentum_buffer"].numpy().ravel()
            assert np.max(np.abs(w - ref_w)) <= 1e-12 * max(1.0, np.max(np.abs(ref_w)))
            assert np.max(np.abs(b - ref_b)) <= 1e-12 * max(1.0, np.max(np.abs(ref_b)))
            assert np.array_equal(one_w[i], w) == bool(is_w[i]), "the second group must show in gamma / beta and nowhere else"
    # the same decay in both groups is the one-group rule, and the flag names a tensor of the whole list
    a = M.sgd_two_groups(mine_w, gs, mine_b, is_w, 0.05, wd, wd, 0.9)
    b = R.step(R.SGD, mine_w, gs, mine_b, is_w, 0.05, wd, 0.9)
    assert all(np.array_equal(x, y) for x, y in zip(a[0] + a[2], b[0] + b[2]))
    gs[2][5] = np.nan
    assert M.sgd_two_groups(mine_w, gs, mine_b, is_w, 0.05, wd, wd_norm, 0.9)[3] == 3


def test_operators_refuse_bad_arguments_before_any_device_work():
    """mi_op_clip_grad_norm: a NULL or misaligned pointer, n == 0, offsets off the 16-byte grid / descending / beyond n, a max_norm that is
    NaN, infinite, zero or negative; mi_op_momentum_update2: a wd_norm that is not finite or negative.  -1 with mi_last_error set, host-side
    checks only: the pointers are never followed (no GPU needed)"""
    from resnet_amd import binding as B
    L = B.load()
    good = (C.c_size_t * 3)(0, 64, 131)
    fake = C.c_void_p(0x10000)
    rec = B.MiClipRecord()
    cases = [(None, 131, good, 2, 1.0), (C.c_void_p(0x10004), 131, good, 2, 1.0), (fake, 0, good, 2, 1.0), (fake, 130, good, 2, 1.0),
             (fake, 131, (C.c_size_t * 3)(0, 62, 131), 2, 1.0), (fake, 131, (C.c_size_t * 3)(64, 0, 131), 2, 1.0), (fake, 131, good, 0, 1.0),
             (fake, 131, None, 2, 1.0), (fake, 2 ** 32, (C.c_size_t * 2)(2 ** 31, 2 ** 31 + 8), 1, 1.0)]
    cases += [(fake, 131, good, 2, m) for m in (float("nan"), float("inf"), 0.0, -1.0)]
    for g, n, off, nt, max_norm in cases:
        L.mi_clear_error()
        assert L.mi_op_clip_grad_norm(g, n, off, nt, max_norm, C.byref(rec)) == -1, (g, n, nt, max_norm)
        assert "mi_op_clip_grad_norm" in L.mi_last_error().decode()
    isw = (C.c_int * 2)(1, 0)
    for wd_norm in (float("nan"), float("inf"), -1e-3):
        L.mi_clear_error()
        assert L.mi_op_momentum_update2(B.MI_OPT_SGD, None, None, None, 131, good, 2, isw, 0.1, 0.0, wd_norm, 0.9, 0.001, None, None) == -1
        assert "wd_norm" in L.mi_last_error().decode()
    L.mi_clear_error()
