"""Gradient accumulation on the device (include/resnet_mi.h, "gradient accumulation"): grad_accum_kernel on its own, the assumption the
design rests on (a backward pass overwrites the gradient arena), a window's values for every optimizer, the off state, the interplay
with running statistics / EMA / loss records / mixing, the data-parallel path, the checkpoint, the refusals and the red zones.  The
model is tests/accumref.py, pinned against torch by tests/test_accum_model.py; comparisons are bit for bit (a NaN that arithmetic
produced matches any NaN, accumref.same).

Kernel lengths are the smallest that cross each path, taken from the launcher's own constants (mi_debug_accum_geometry); the trainer
runs on the small nets of tests/synth.py, ResNet-50 at batch 2 only where the issue is every kernel route of the real network.
"""
import ctypes as C
import os

import numpy as np
import pytest

import accumref as M
import mixref as R
import synth

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
FIRST, ADD, FOLD = M.FIRST, M.ADD, M.FOLD
MODES = [(FIRST, "first"), (ADD, "add"), (FOLD, "fold")]
GUARD = 16
FILL = np.float32(-12345.5)
SCALE = np.float32(1.0) / np.float32(3.0)
NETS = {"C1S": (synth.C1S_DIMS, 4), "C1S_batch5": (synth.C1S_DIMS, 5), "C4I": (synth.C4I_DIMS, 4), "R50": (synth.R50_DIMS, 2)}
_PARAMS = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _pair(n, seed):
    """an accumulator and a gradient of mixed magnitude, with elements that cancel exactly and zeros of both signs"""
    rng = np.random.RandomState(seed)
    acc = (rng.randn(n) * 10.0 ** rng.randint(-4, 4, size=n)).astype(np.float32)
    g = (rng.randn(n) * 10.0 ** rng.randint(-4, 4, size=n)).astype(np.float32)
    for k, at in enumerate(range(0, n, 97)):
        g[at] = (-acc[at], 0.0, -0.0)[k % 3]
    return acc, g


def _model(mode, acc, g, scale):
    """(acc, g) after the launch"""
    if mode == FIRST:
        return M.first(g), g
    if mode == ADD:
        return M.add(acc, g), g
    return acc, M.fold(acc, g, scale)


def _lengths(ops, offset):
    _, turn_v, turn_e, cap = ops.accum_geometry()
    turn = turn_e if offset else turn_v
    return sorted({1, 3, 4, 5, 1023, 1024, 1025, turn - 1, turn, turn + 1}), cap * turn + turn + turn // 2 + 3


def _guards_ok(res):
    return all(g.size == GUARD and np.all(g == FILL) for g in res[1:])


def _check_launch(ops, mode, offset, acc, g, scale, what):
    got_acc, got_g = ops.grad_accumulate(acc, g, mode, scale, offset_floats=offset, guard=GUARD, fill=FILL)
    want_acc, want_g = _model(mode, acc, g, scale)
    for got, want, name in ((got_acc, want_acc, "acc"), (got_g, want_g, "g")):
        bad = int(np.sum((_bits(got[0]) != _bits(want)) & ~(np.isnan(got[0]) & np.isnan(want))))
        assert bad == 0 and M.same(got[0], want), "%s: %d elements of %s differ from the model" % (what, bad, name)
        assert _guards_ok(got), "%s: a guard word of %s was written" % (what, name)
    # the operand that is only read keeps its bits, and FIRST is a copy of words
    if mode == FOLD:
        assert _same(got_acc[0], acc), what + ": FOLD wrote acc"
    else:
        assert _same(got_g[0], g), what + ": g was written"
    if mode == FIRST:
        assert _same(got_acc[0], g), what + ": FIRST is the words of g"
    return got_acc[0], got_g[0]


# ---- 1. the kernel on its own ----
def test_geometry_is_the_ema_kernels(ops):
    assert ops.accum_geometry() == ops.ema_geometry() and ops.accum_geometry()[0] == 256


@pytest.mark.parametrize("offset", [0, 1], ids=["vector", "element-wise"])
@pytest.mark.parametrize("mode", [m for m, _ in MODES], ids=[n for _, n in MODES])
def test_kernel_is_the_model(ops, mode, offset):
    lengths, second = _lengths(ops, offset)
    for n in lengths + [second]:  # the last: a second grid-stride turn behind the capped grid
        acc, g = _pair(n, n % 1000)
        _check_launch(ops, mode, offset, acc, g, SCALE, "n = %d" % n)


@pytest.mark.parametrize("offset", [0, 1], ids=["vector", "element-wise"])
@pytest.mark.parametrize("mode", [m for m, _ in MODES], ids=[n for _, n in MODES])
def test_tails_and_partial_turns_on_inputs_that_separate_the_alternatives(ops, mode, offset):
    """the lengths above on accumref.separating_pair: EVERY element tells the fold (a sum, then a product) from the fold rounded once,
    and acc != g everywhere, so that the n % 4 tail and the partial turn, which have their own lines in the kernel, cannot round
    differently or read an operand twice unnoticed.  _pair's inputs separate about a quarter of the elements (tests/test_accum_model.py
    holds the 100 % as a condition, without a GPU)"""
    import emaref
    _, turn_v, turn_e, _ = ops.accum_geometry()
    for n in _lengths(ops, offset)[0]:
        acc, g = M.separating_pair(n, SCALE, n)
        at = emaref.tail_and_partial_turn(n, turn_e if offset else turn_v, not offset)
        assert np.all(_bits(M.fold(acc, g, SCALE))[at] != _bits(M.fold_once(acc, g, SCALE))[at]) and np.all(acc[at] != g[at])
        _check_launch(ops, mode, offset, acc, g, SCALE, "n = %d" % n)


@pytest.mark.parametrize("offset", [0, 1], ids=["vector", "element-wise"])
@pytest.mark.parametrize("mode", [m for m, _ in MODES], ids=[n for _, n in MODES])
def test_kernel_propagates_what_is_not_finite(ops, mode, offset):
    """NaN (with a payload), +-inf, -0 and a denormal in the vector body, in the n % 4 tail and in the second grid-stride turn, in either
    operand: IEEE results, no guard; FIRST keeps every bit"""
    lengths, n = _lengths(ops, offset)
    turn = lengths[-2]
    words = np.array([0x7FC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0xFFC00001, 0x7F800001], np.uint32).view(np.float32)
    tail = [n - 3, n - 2, n - 1] if not offset else []  # the n % 4 words behind the last 16-byte group
    assert offset or n % 4 == 3
    spots = list(range(8, 8 + len(words))) + [turn + 2, n // 2] + list(range(n - turn // 2, n - turn // 2 + len(words))) + tail
    denormal = np.float32(1e-40)
    for where in ("g", "acc", "both"):
        acc, g = _pair(n, 3)
        for i, at in enumerate(spots):
            if where in ("g", "both"):
                g[at] = words[i % len(words)]
            if where in ("acc", "both"):
                acc[at] = words[(i + 3) % len(words)]
        acc[20], g[20], acc[n - 5], g[n - 5] = denormal, denormal, -denormal, denormal / 4  # sums and products that stay denormal
        got_acc, got_g = _check_launch(ops, mode, offset, acc, g, SCALE, "planted in %s" % where)
        if mode != FIRST:
            assert (got_g if mode == FOLD else got_acc)[20] != 0, "a denormal result was flushed"
    # inf + -inf, and a sum that overflows: NaN and inf, not a kept value
    acc, g = _pair(64, 9)
    acc[3], g[3] = np.inf, -np.inf
    acc[7], g[7] = np.float32(3e38), np.float32(3e38)
    got_acc, got_g = _check_launch(ops, mode, offset, acc, g, SCALE, "inf - inf")
    if mode != FIRST:
        out = got_g if mode == FOLD else got_acc
        assert np.isnan(out[3]) and np.isposinf(out[7])


def test_fold_rounds_the_sum_and_the_product_separately(ops):
    rng = np.random.RandomState(7)
    a, b = rng.randn(4096).astype(np.float32), (rng.randn(4096) * 1e-4).astype(np.float32)
    once = ((a.astype(np.float64) + b.astype(np.float64)) * np.float64(SCALE)).astype(np.float32)
    for offset in (0, 1):
        _, got = ops.grad_accumulate(a, b, FOLD, SCALE, offset_floats=offset)
        assert _same(got, M.fold(a, b, SCALE)) and not _same(got, once)


def test_operator_refusals(ops):
    L = ops.L
    acc, g = _pair(64, 1)
    da, dg = ops.dev(acc), ops.dev(g)

    def refused(rc, word):
        try:
            assert rc == -1 and word in L.mi_last_error().decode(), (rc, L.mi_last_error())
        finally:
            L.mi_clear_error()

    for mode in (FIRST, ADD, FOLD):
        refused(L.mi_op_grad_accumulate(None, dg.ptr, 64, mode, 1.0), "NULL")
        refused(L.mi_op_grad_accumulate(da.ptr, None, 64, mode, 1.0), "NULL")
        refused(L.mi_op_grad_accumulate(da.ptr + 2, dg.ptr, 8, mode, 1.0), "4-byte aligned")
        refused(L.mi_op_grad_accumulate(da.ptr, dg.ptr + 1, 8, mode, 1.0), "4-byte aligned")
        refused(L.mi_op_grad_accumulate(da.ptr, dg.ptr, 0, mode, 1.0), "n lies in")
        refused(L.mi_op_grad_accumulate(da.ptr, dg.ptr, (1 << 40) + 1, mode, 1.0), "n lies in")
        refused(L.mi_op_grad_accumulate(da.ptr, da.ptr + 4 * 16, 17, mode, 1.0), "overlap")
        refused(L.mi_op_grad_accumulate(da.ptr + 4 * 16, da.ptr, 17, mode, 1.0), "overlap")
        refused(L.mi_op_grad_accumulate(da.ptr, da.ptr, 4, mode, 1.0), "overlap")
    for mode in (-1, 3, 7):
        refused(L.mi_op_grad_accumulate(da.ptr, dg.ptr, 64, mode, 1.0), "unknown mode")
    for scale in (0.0, -0.5, float("nan"), float("inf"), float("-inf")):
        refused(L.mi_op_grad_accumulate(da.ptr, dg.ptr, 64, FOLD, scale), "scale")
    assert _same(da.get(), acc) and _same(dg.get(), g), "a refused call wrote something"
    # the scale is FOLD's alone, and adjacent ranges are fine
    assert L.mi_op_grad_accumulate(da.ptr, dg.ptr, 64, ADD, float("nan")) == 0
    assert _same(da.get(), M.add(acc, g)) and _same(dg.get(), g)
    assert L.mi_op_grad_accumulate(dg.ptr, dg.ptr + 4 * 16, 16, FIRST, 0.0) == 0
    assert _same(dg.get(), np.concatenate([g[16:32], g[16:]]))


# ---- the trainer ----
def _params(dims):
    key = (dims["input"], dims["n_conv_blocks"], tuple(dims["is_block_spatial_reduction"]))
    if key not in _PARAMS:
        _PARAMS[key] = synth.make_params(dims, perturb_bn=True)
    return _PARAMS[key]


def _trainer(dims, batch, dtype=F32, params=None, **kw):
    from resnet_amd import Trainer
    from resnet_amd import binding as B
    tr = Trainer(dims, batch, **kw)
    if tr.L.mi_device_count() < 1:
        pytest.fail("no HIP device: this test must run on the MI355X box")
    tr.set_dtype(dtype)
    tr.set_params(params if params is not None else _params(dims))
    tr.source_host(B.MI_LAYOUT_NHWC)
    return tr


def _load(tr, dims, batch, step):
    im, lab = synth.make_batch(dims, batch, step=step)
    tr.fill_host_batch(im, lab)
    tr.load_new_batch()


def _fwd_bwd(tr, dims, batch, step):
    _load(tr, dims, batch, step)
    tr.forward()
    tr.backward()
    tr.check()


def _all(tr, which):
    return [tr.get(which, i) for i in range(tr.n_locations)]


def _state(tr):
    """parameters, both moment arenas, the decays"""
    t = tr.t.contents
    return _all(tr, "params") + _all(tr, "means") + _all(tr, "vars") + [np.array([t.cur_mean_decay, t.cur_var_decay], np.float32)]


def _assert_lists_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        bad = int(np.sum(_bits(g) != _bits(w))) if g.shape == w.shape else -1
        assert bad == 0, "%s: entry %d: %d elements differ" % (what, i, bad)


def _grad_offsets(tr):
    """float offsets of the locations[] tensors in the gradient arena (every arena has them)"""
    p = tr._pset("grads")
    base = C.cast(p.locations[0], C.c_void_p).value
    return [(C.cast(p.locations[i], C.c_void_p).value - base) // 4 for i in range(tr.n_locations)]


def _grad_arena(tr):
    return C.cast(tr._pset("grads").locations[0], C.c_void_p).value, int(tr.L.mi_debug_arena_floats(tr.c_dims))


# ---- 2. the assumption the design rests on: a backward pass overwrites the gradient arena ----
@pytest.mark.parametrize("case", [("C1S_batch5", F32), ("C4I", BF16), ("R50", F32), ("R50", BF16)], ids=["C1S_batch5-f32", "C4I-bf16", "R50-f32", "R50-bf16"])
def test_backward_overwrites_a_poisoned_gradient_arena(case):
    """passes without accumulation too: it keeps the assumption true.  Every byte of the arena 0xFF (NaN words) before forward and
    backward; every element of every gradient tensor then holds the bits of a run from a zeroed arena"""
    net, dtype = case
    dims, batch = NETS[net]
    tr = _trainer(dims, batch, dtype)
    try:
        base, floats = _grad_arena(tr)
        runs = []
        for byte in (0x00, 0xFF):
            fill = np.full(floats * 4, byte, np.uint8)
            tr.L.mi_copy_to_device(base, fill.ctypes.data, fill.nbytes)
            _fwd_bwd(tr, dims, batch, 0)
            tr.L.mi_device_synchronize()
            runs.append(_all(tr, "grads"))
        for i, (zeroed, poisoned) in enumerate(zip(*runs)):
            assert not np.any(np.isnan(poisoned)), "location %d: %d NaN survive the backward pass" % (i, int(np.isnan(poisoned).sum()))
            assert _same(zeroed, poisoned), "location %d: %d elements depend on what the arena held" % (i, int(np.sum(_bits(zeroed) != _bits(poisoned))))
        assert any(np.any(g != 0) for g in runs[0])
    finally:
        tr.close()


# ---- 3. values of a window ----
def _copy_state(src, dst):
    for which in ("params", "means", "vars"):
        for i in range(src.n_locations):
            dst.set(which, i, src.get(which, i))
    dst.t.contents.cur_mean_decay = src.t.contents.cur_mean_decay
    dst.t.contents.cur_var_decay = src.t.contents.cur_var_decay


def _plant_nan_in_accumulator(ops, tr):
    acc = tr.L.mi_debug_accum_arena(tr.t)
    assert acc
    nan = ops.dev(np.full(max(tr.sizes), np.nan, np.float32))
    back = np.empty(max(tr.sizes), np.float32)
    for off, size in zip(_grad_offsets(tr), tr.sizes):
        assert tr.L.mi_op_grad_accumulate(acc + 4 * off, nan.ptr, size, FIRST, 1.0) == 0, tr.error()
        tr.L.mi_copy_to_host(back.ctypes.data, acc + 4 * off, 4 * size)
        assert np.all(np.isnan(back[:size]))
    nan.free()


WINDOW_CASES = [("C1S", F32, 2), ("C1S", F32, 3), ("C4I", BF16, 2)]


@pytest.mark.parametrize("optim", ["adam", "sgd", "lars"])
@pytest.mark.parametrize("case", WINDOW_CASES, ids=["%s-%s-k%d" % (n, ("f32", "bf16")[d], k) for n, d, k in WINDOW_CASES])
def test_a_window_is_one_update_on_the_folded_gradient(ops, case, optim):
    """trainer A accumulates; trainer B, accumulation off, gets A's state and the model's folded gradient and runs one update_parameters.
    Window 1 at scale 1, window 2 at scale 0.5 and from an accumulator full of NaN: the window starts with FIRST"""
    net, dtype, k = case
    dims, batch = NETS[net]
    kw = dict(lr=1e-3, wd=1e-4)
    a, b = _trainer(dims, batch, dtype, **kw), _trainer(dims, batch, dtype, **kw)
    try:
        for tr in (a, b):
            if optim != "adam":
                tr.set_optimizer(optim, momentum=0.9)
        a.track_running_stats(0.1)
        a.set_ema(0.5, every=1)
        assert a.accumulation() == (1, 0)
        step = 0
        for window, scale in enumerate((1.0, 0.5)):
            a.set_accumulation(k, scale)
            if window == 1:
                _plant_nan_in_accumulator(ops, a)
            grads = []
            for j in range(1, k + 1):
                _fwd_bwd(a, dims, batch, step)
                step += 1
                grads.append(_all(a, "grads"))
                if j < k:
                    before = _state(a), [a.ema_get(i) for i in range(a.n_locations)], a.ema_updates()
                    a.update()
                    assert a.check_errors() == 0
                    _assert_lists_same(_state(a), before[0], "window %d, collecting call %d: parameters, moments, decays" % (window, j))
                    _assert_lists_same([a.ema_get(i) for i in range(a.n_locations)], before[1], "collecting call %d: the EMA" % j)
                    assert a.ema_updates() == before[2] == window and a.accumulation() == (k, j)
            want = [M.window([g[i] for g in grads], np.float32(scale)) for i in range(a.n_locations)]
            assert all(np.all(np.isfinite(w)) for w in want) and any(np.any(w != 0) for w in want)
            _copy_state(a, b)
            for i, w in enumerate(want):
                b.set("grads", i, w)
            b.update()
            a.update()
            assert a.check_errors() == 0 and b.check_errors() == 0
            assert a.accumulation() == (k, 0) and a.ema_updates() == window + 1
            got, ref = _state(a), _state(b)
            _assert_lists_same(got, ref, "%s, window %d: A's applying call against B's update on the folded gradient" % (optim, window))
            assert all(np.all(np.isfinite(x)) for x in got)
            assert any(not _same(x, y) for x, y in zip(got[:a.n_locations], before[0][:a.n_locations])), "the update moved nothing"
            _assert_lists_same(_all(a, "grads"), _all(b, "grads"), "the gradient arena behind the optimizer")
    finally:
        a.close()
        b.close()


# ---- 4. off is off ----
def _ring(L, may_be_empty=False):
    buf = C.create_string_buffer(1 << 16)
    n = L.mi_debug_trace_names(buf, len(buf))
    names = buf.value.decode().split("\n")[:-1]
    assert (0 if may_be_empty else 1) <= n == len(names) < 96, "the launch ring is off, or full (%d): launches were lost" % n
    return names


def test_off_is_off():
    dims, batch = NETS["C1S"]
    runs = []
    for call in (None, 1):
        tr = _trainer(dims, batch)
        try:
            if call:
                tr.set_accumulation(1, 1.0)
            assert tr.accumulation() == (1, 0) and not tr.L.mi_debug_accum_arena(tr.t)
            names = []
            for step in range(3):
                for phase in (lambda: _load(tr, dims, batch, step), tr.forward, tr.backward, tr.update):
                    tr.L.mi_debug_trace_clear()
                    phase()
                    names.append(_ring(tr.L, may_be_empty=True))
                assert tr.accumulation() == (1, 0)
            assert tr.check_errors() == 0
            runs.append((_state(tr), names, tr.device_bytes()))
        finally:
            tr.close()
    _assert_lists_same(runs[1][0], runs[0][0], "set_accumulation(1, 1.0) against never calling it")
    assert runs[1][1] == runs[0][1] and runs[1][2] == runs[0][2]
    assert not [n for phase in runs[0][1] for n in phase if "accum" in n]
    # ... and a trainer that has the accumulator but is back at k = 1 computes the same, with the arena still counted
    tr = _trainer(dims, batch)
    try:
        tr.set_accumulation(2, 0.5)
        tr.set_accumulation(1, 1.0)
        for step in range(3):
            _fwd_bwd(tr, dims, batch, step)
            tr.update()
        assert tr.check_errors() == 0
        _assert_lists_same(_state(tr), runs[0][0], "k back at 1")
        assert tr.device_bytes() - runs[0][2] == 4 * tr.L.mi_debug_arena_floats(tr.c_dims)
    finally:
        tr.close()


def test_a_collecting_update_launches_one_kernel_and_keeps_the_weights_laid_out():
    dims, batch = NETS["C1S"]
    tr = _trainer(dims, batch)
    try:
        tr.set_accumulation(3, 1.0)
        want = ["grad_accum_kernel<first,vector>", "grad_accum_kernel<add,vector>", "grad_accum_kernel<fold,vector>"]
        fwd = []
        for j in range(4):
            _load(tr, dims, batch, j)
            tr.L.mi_debug_trace_clear()
            tr.forward()
            fwd.append(_ring(tr.L))
            tr.backward()
            tr.L.mi_debug_trace_clear()
            tr.update()
            names = _ring(tr.L)
            assert [n for n in names if "accum" in n] == [want[j % 3]]
            assert (len(names) == 1) == (j % 3 < 2), names
            assert tr.timings()[3] > 0
        assert tr.check_errors() == 0
        # the forward passes behind a collecting call re-lay no weights; the one behind the applying call does what the first did
        assert fwd[1] == fwd[2] and fwd[3] == fwd[0] and (fwd[1] == fwd[0] or len(fwd[1]) < len(fwd[0]))
    finally:
        tr.close()


# ---- 5. interplay ----
def _mix_seed(dim, steps):
    for seed in range(1000):
        ps = [R.plan(seed, 0, s, 0, 1, 0.8, 1.0, 1.0, 0.5, dim) for s in steps]
        if ps[0] != ps[1] and ps[2] != ps[3] and all(p["mode"] != 0 for p in ps):
            return seed, ps
    raise AssertionError("no such seed")


def test_interplay_with_running_statistics_ema_loss_records_and_mixing():
    dims, batch = NETS["C1S"]
    seed, plans = _mix_seed(dims["input"], range(-1, 3))  # the plan's step is cur_dump_id before its increment: -1 at the first load
    tr = _trainer(dims, batch, lr=1e-3)
    try:
        tr.set_optimizer("sgd", momentum=0.9)
        tr.track_running_stats(0.1)
        tr.set_ema(0.5, every=1)
        tr.set_loss(smoothing=0.1, topk=5, device=True)
        tr.set_mix(mixup=0.8, cutmix=1.0, prob=1.0, switch=0.5, seed=seed)
        tr.set_accumulation(2, 0.5)
        seen = []
        for step in range(4):
            _load(tr, dims, batch, step)
            seen.append(tr.last_mix())
            tr.forward()
            tr.backward()
            tr.update()
            assert tr.accumulation() == (2, (step + 1) % 2) and tr.ema_updates() == (step + 1) // 2
        assert tr.check_errors() == 0
        assert tr.running_updates() == 4 and tr.ema_updates() == 2
        last, total = tr.metrics()
        assert total["batches"] == 4 and total["rows"] == 4 * batch and last["rows"] == batch
        for got, want in zip(seen, plans):
            assert all(got[key] == want[key] for key in ("mode", "y0", "x0", "y1", "x1")) and np.float32(got["lam"]) == np.float32(want["lam"])
        assert seen[0] != seen[1] and seen[2] != seen[3], "every micro-batch of a window draws its own plan"
    finally:
        tr.close()


# ---- 6. data parallel, a one-rank communicator ----
_DP_RUNS = {}


def _dp_run(overlap, with_comm):
    """one k = 2 window on C4I in a weight-gradient overlap mode, with or without a one-rank communicator (all-reduce = identity) whose
    buckets are small enough that there are several; the state behind it.  Computed once per (overlap, with_comm)"""
    if (overlap, with_comm) in _DP_RUNS:
        return _DP_RUNS[overlap, with_comm]
    dims, batch = NETS["C4I"]
    tr = _trainer(dims, batch, lr=1e-3)
    try:
        tr.L.mi_trainer_set_overlap(tr.t, overlap)
        if with_comm:
            nbytes = tr.L.mi_dp_unique_id_bytes()
            uid = (C.c_char * nbytes)()
            assert tr.L.mi_dp_get_unique_id(uid, nbytes) == 0, tr.error()
            assert tr.L.mi_dp_init(tr.t, 0, 1, uid, nbytes) == 0, tr.error()
            tr.L.mi_dp_set_bucket_bytes(tr.t, 256 << 10)
        tr.set_accumulation(2, 0.5)
        fr, to = (C.c_size_t * 64)(), (C.c_size_t * 64)()
        _fwd_bwd(tr, dims, batch, 0)
        assert tr.L.mi_debug_last_buckets(tr.t, fr, to, 64) == 0, "a collecting backward cut a bucket"
        tr.update()
        assert tr.accumulation() == (2, 1)
        _fwd_bwd(tr, dims, batch, 1)
        nb = tr.L.mi_debug_last_buckets(tr.t, fr, to, 64)
        if with_comm:
            assert nb >= 2 and to[0] == tr.L.mi_debug_arena_floats(tr.c_dims) and fr[nb - 1] == 0
            assert all(fr[i] == to[i + 1] for i in range(nb - 1)), "the buckets tile the arena"
        else:
            assert nb == 0
        tr.update()
        assert tr.check_errors() == 0 and tr.accumulation() == (2, 0)
        _DP_RUNS[overlap, with_comm] = _state(tr)
    finally:
        tr.close()
    return _DP_RUNS[overlap, with_comm]


@pytest.mark.parametrize("overlap", [0, 1, 2])
def test_data_parallel_one_rank_folds_bucket_by_bucket(overlap):
    """the collecting backward cuts no bucket, the applying one folds each in front of its all-reduce, and update_parameters does not fold
    again: the bits of the run without a communicator, and of weight-gradient overlap mode 0"""
    dims, _ = NETS["C4I"]
    plain = _dp_run(overlap, False)
    _assert_lists_same(_dp_run(overlap, True), plain, "overlap %d: with / without a communicator" % overlap)
    _assert_lists_same(plain, _dp_run(0, False), "overlap %d against overlap 0" % overlap)
    assert any(not _same(x, y) for x, y in zip(plain, _params(dims)))


# ---- 7. checkpoint ----
def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_checkpoint(tmp_path, capfd):
    dims, batch = NETS["C1S"]
    K = 3
    listing, grads, straight = {}, [], None
    for name, k in (("plain", 1), ("accum", K)):
        tr = _trainer(dims, batch, dump_dir="ck", lr=1e-3)
        try:
            root = str(tmp_path / name)
            tr.L.mi_trainer_set_dump_root(tr.t, root.encode())
            tr.set_accumulation(k, 0.5)
            _fwd_bwd(tr, dims, batch, 0)  # (every tensor a dump holds has been written)
            tr.L.dump_trainer(1, tr.t, b"ck")  # pending == 0: what a trainer without accumulation writes
            tr.check()
            if k > 1:
                for step in range(2):
                    if step:
                        _fwd_bwd(tr, dims, batch, step)
                    grads.append(_all(tr, "grads"))
                    tr.update()
                assert tr.accumulation() == (K, 2)
                tr.L.dump_trainer(2, tr.t, b"ck")
                tr.check()
                _fwd_bwd(tr, dims, batch, 2)
                tr.update()
                assert tr.check_errors() == 0 and tr.accumulation() == (K, 0)
                straight = _state(tr)
            listing[name] = _files(root)
        finally:
            tr.close()
    d1, d2 = os.path.join("ck", "%08d" % 1), os.path.join("ck", "%08d" % 2)
    in1 = [f for f in listing["accum"] if f.startswith(d1)]
    assert in1 == listing["plain"] and not [f for f in in1 if "accum" in f]
    for f in in1:
        assert open(str(tmp_path / "accum" / f), "rb").read() == open(str(tmp_path / "plain" / f), "rb").read(), f
    in2 = [os.path.relpath(f, d2) for f in listing["accum"] if f.startswith(d2)]
    assert sorted(set(in2) - {os.path.relpath(f, d1) for f in in1}) == ["grad_accum.buffer"]
    raw = open(str(tmp_path / "accum" / d2 / "grad_accum.buffer"), "rb").read()
    arena = None
    tr = _trainer(dims, batch, dump_dir="ck", lr=1e-3)
    try:
        arena = int(tr.L.mi_debug_arena_floats(tr.c_dims))
        assert len(raw) == 8 + 4 * arena and list(np.frombuffer(raw[:8], np.int32)) == [K, 2]
        held = np.frombuffer(raw[8:], np.float32)
        covered = np.zeros(arena, bool)
        for i, (off, size) in enumerate(zip(_grad_offsets(tr), tr.sizes)):
            assert _same(held[off:off + size], M.accumulator([grads[0][i], grads[1][i]])), "location %d of the dumped accumulator" % i
            covered[off:off + size] = True
        assert np.all(_bits(held)[~covered] == 0), "padding words"
        # a fresh trainer, restored inside the window, finishes it on the same third batch
        capfd.readouterr()
        tr.L.mi_trainer_set_dump_root(tr.t, str(tmp_path / "accum").encode())
        tr.set_accumulation(K, 0.5)
        tr.L.overwrite_model_params(tr.t, 2, b"ck")
        tr.L.overwrite_trainer_hyperparams(tr.t, 2, b"ck")
        tr.check()
        assert tr.accumulation() == (K, 2) and "grad_accum" not in capfd.readouterr().err
        _fwd_bwd(tr, dims, batch, 2)
        tr.update()
        assert tr.check_errors() == 0 and tr.accumulation() == (K, 0)
        _assert_lists_same(_state(tr), straight, "the window finished after a restore against the straight run")
        # a dump without the file: pending 0, no note
        _fwd_bwd(tr, dims, batch, 3)
        tr.update()
        assert tr.accumulation() == (K, 1)
        tr.L.overwrite_model_params(tr.t, 1, b"ck")
        assert tr.accumulation() == (K, 0) and "grad_accum" not in capfd.readouterr().err
    finally:
        tr.close()
    # another k: pending 0 and one note
    tr = _trainer(dims, batch, dump_dir="ck")
    try:
        tr.L.mi_trainer_set_dump_root(tr.t, str(tmp_path / "accum").encode())
        tr.set_accumulation(K + 1, 0.5)
        tr.L.overwrite_model_params(tr.t, 2, b"ck")
        err = capfd.readouterr().err
        assert tr.accumulation() == (K + 1, 0) and err.count("grad_accum.buffer") == 1, err
        tr.set_accumulation(1, 1.0)  # off: the file is not looked at
        tr.L.overwrite_model_params(tr.t, 2, b"ck")
        assert tr.accumulation() == (1, 0) and "grad_accum" not in capfd.readouterr().err
    finally:
        tr.close()


# ---- 8. refusals ----
def test_trainer_refusals():
    dims, batch = NETS["C1S"]
    tr = _trainer(dims, batch)
    L, t = tr.L, tr.t

    def refused(rc, word):
        try:
            assert rc == -1 and word in tr.error(), (rc, tr.error())
        finally:
            L.mi_clear_error()

    try:
        before = tr.device_bytes()
        for k in (0, -1):
            refused(L.mi_trainer_set_accumulation(t, k, 1.0), "k is >= 1")
        for scale in (0.0, -1.0, float("nan"), float("inf")):
            refused(L.mi_trainer_set_accumulation(t, 2, scale), "scale")
        assert tr.accumulation() == (1, 0) and tr.device_bytes() == before and not L.mi_debug_accum_arena(t), "a refused call allocated or set something"
        tr.set_accumulation(2, 0.5)
        assert tr.device_bytes() - before == 4 * L.mi_debug_arena_floats(tr.c_dims)
        tr.set_accumulation(4, 0.25)  # between windows: as often as one likes, one arena
        assert tr.accumulation() == (4, 0) and tr.device_bytes() - before == 4 * L.mi_debug_arena_floats(tr.c_dims)
        _load(tr, dims, batch, 0)
        tr.forward()
        refused(L.mi_trainer_set_accumulation(t, 2, 1.0), "between forward_pass and update_parameters")
        tr.backward()
        refused(L.mi_trainer_set_accumulation(t, 2, 1.0), "between forward_pass and update_parameters")
        tr.update()
        assert tr.accumulation() == (4, 1)
        for k in (1, 2, 4):
            refused(L.mi_trainer_set_accumulation(t, k, 1.0), "pending")
        with pytest.raises(RuntimeError, match="pending"):
            tr.set_accumulation(2)
        assert tr.accumulation() == (4, 1)
        for step in range(1, 4):
            _fwd_bwd(tr, dims, batch, step)
            tr.update()
        assert tr.accumulation() == (4, 0), "a refused call changed k"
        tr.set_accumulation(1, 1.0)
        assert tr.check_errors() == 0
    finally:
        tr.close()


# ---- 9. red zones ----
def test_red_zones_around_a_window(ops):
    L = ops.L
    dims, batch = NETS["C1S_batch5"]
    assert L.mi_debug_redzone(4096, 0xFF) == 0
    try:
        tr = _trainer(dims, batch, BF16)
        try:
            tr.set_optimizer("lars", momentum=0.9)
            tr.set_accumulation(2, 0.5)
            for step in range(2):
                _fwd_bwd(tr, dims, batch, step)
                tr.update()
            assert tr.check_errors() == 0 and tr.accumulation() == (2, 0)
            assert L.mi_debug_redzone_check() == 0, tr.error()
        finally:
            tr.close()
        assert L.mi_debug_redzone_check() == 0, L.mi_last_error()
        checked, live = C.c_size_t(0), C.c_size_t(0)
        L.mi_debug_redzone_stats(C.byref(checked), None, C.byref(live))
        assert checked.value > 0
    finally:
        L.mi_debug_redzone(0, 0)
