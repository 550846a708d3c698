"""Weight averaging on the device (include/resnet_mi.h, "weight averaging"): the EMA and the exchange kernel on their own, the EMA
behind update_parameters, evaluation on the averaged model, the checkpoint.  The model is tests/emaref.py, pinned against torch.lerp by
tests/test_ema_model.py; every comparison here is bit for bit.

Every test calls a symbol the library did not have before.  Kernel lengths are the smallest that cross each path (the n % 4 tail, one
workgroup's unrolled turn +- 1, a second grid-stride turn behind the capped grid), taken from the launcher's own constants
(mi_debug_ema_geometry); the trainer runs on the small nets of tests/synth.py and on ResNet-50 at batch 2.
"""
import ctypes as C
import os

import numpy as np
import pytest

import emaref as M
import evalref as E
import synth
import torch_ref as T

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
GUARD = 16
FILL = np.float32(-12345.5)
WEIGHTS = [M.weight(0.9999, False, 0), np.float32(0.1), np.float32(0.5), np.float32(0.8), np.float32(1.0)]
NETS = {"C1S": (synth.C1S_DIMS, 4), "C1S_batch5": (synth.C1S_DIMS, 5), "C4I": (synth.C4I_DIMS, 4), "R50": (synth.R50_DIMS, 2)}
CASES = [("C1S_batch5", F32), ("C4I", BF16), ("R50", BF16)]
CASE_IDS = ["%s-%s" % (n, ("f32", "bf16")[d]) for n, d in CASES]
_PARAMS = {}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _pair(n, seed):
    """the inputs of the model test, with a few elements where p == e (a zero and a -0 among them)"""
    rng = np.random.RandomState(seed)
    e = (0.1 * rng.randn(n)).astype(np.float32)
    p = (e + 0.01 * rng.randn(n)).astype(np.float32)
    for k, at in enumerate(range(0, n, 97)):
        e[at] = (0.0, -0.0, e[at])[k % 3]
        p[at] = e[at]
    return e, p


def _lengths(ops, offset):
    _, turn_v, turn_e, _ = ops.ema_geometry()
    turn = turn_e if offset else turn_v
    return sorted({1, 3, 4, 5, 1023, 1024, 1025, turn - 1, turn, turn + 1})


def _second_turn_length(ops, offset):
    """behind a whole sweep of the capped grid: workgroup 0 takes a whole second turn, workgroup 1 half a turn, and 3 elements remain"""
    _, turn_v, turn_e, cap = ops.ema_geometry()
    turn = turn_e if offset else turn_v
    return cap * turn + turn + turn // 2 + 3


def _guards_ok(res):
    return all(g.size == GUARD and np.all(g == FILL) for g in res[1:])


# ---- 1. the kernels on their own ----
@pytest.mark.parametrize("w", WEIGHTS, ids=["w=%g" % w for w in WEIGHTS])
@pytest.mark.parametrize("offset", [0, 1], ids=["vector", "element-wise"])
def test_ema_kernel_is_the_model(ops, offset, w):
    for n in _lengths(ops, offset):
        e, p = _pair(n, n)
        got_e, got_p = ops.ema_update(e, p, w, offset_floats=offset, guard=GUARD, fill=FILL)
        want = M.lerp32(e, p, w)
        bad = int(np.sum(_bits(got_e[0]) != _bits(want)))
        assert bad == 0, "n = %d: %d elements differ from the model" % (n, bad)
        assert _same(got_p[0], p) and _guards_ok(got_e) and _guards_ok(got_p), "n = %d: p or a guard word was written" % n
        if w == 1.0:
            assert _same(got_e[0], p), "w = 1: p's bits"
        same = p == e
        assert np.array_equal(got_e[0][same], e[same]), "p == e: the value stays"


@pytest.mark.parametrize("w", [np.float32(0.1), np.float32(0.8), np.float32(0.5)], ids=["w=0.1", "w=0.8", "w=0.5"])
@pytest.mark.parametrize("offset", [0, 1], ids=["vector", "element-wise"])
def test_ema_tails_and_partial_turns_on_inputs_that_separate_the_alternatives(ops, offset, w):
    """the lengths above on emaref.separating_pair: EVERY element tells the model from the wrong kernel this weight is there to catch
    (the unfused update at 0.1 and 0.8, the other branch at 0.5), so that the n % 4 tail (1 to 3 elements) and the partial turn, which
    have their own lines in the kernel, cannot be written with another rounding unnoticed.  _pair's inputs separate 2 to 6 % of the
    elements, and none at n <= 5 (tests/test_ema_model.py holds the 100 % as a condition, without a GPU)"""
    _, turn_v, turn_e, _ = ops.ema_geometry()
    for n in _lengths(ops, offset):
        e, p = M.separating_pair(n, w, n)
        want = M.lerp32(e, p, w)
        at = M.tail_and_partial_turn(n, turn_e if offset else turn_v, not offset)
        assert np.all(_bits(want)[at] != _bits(M.alternative32(e, p, w))[at])
        got_e, got_p = ops.ema_update(e, p, w, offset_floats=offset, guard=GUARD, fill=FILL)
        bad = _bits(got_e[0]) != _bits(want)
        assert not bad.any(), "n = %d: %d elements differ from the model, %d of them in the tail or the partial turn" % (n, int(bad.sum()), int(bad[at].sum()))
        assert _same(got_p[0], p) and _guards_ok(got_e) and _guards_ok(got_p), "n = %d: p or a guard word was written" % n


@pytest.mark.parametrize("offset", [0, 1], ids=["vector", "element-wise"])
def test_ema_and_exchange_take_a_second_grid_stride_turn(ops, offset):
    n = _second_turn_length(ops, offset)
    e, p = _pair(n, 11)
    got_e, got_p = ops.ema_update(e, p, np.float32(0.1), offset_floats=offset, guard=GUARD, fill=FILL)
    bad = int(np.sum(_bits(got_e[0]) != _bits(M.lerp32(e, p, np.float32(0.1)))))
    assert bad == 0, "%d of %d elements differ from the model" % (bad, n)
    assert _same(got_p[0], p) and _guards_ok(got_e) and _guards_ok(got_p)
    a, b = ops.exchange(e, p, offset_floats=offset, guard=GUARD, fill=FILL)
    assert _same(a[0], p) and _same(b[0], e) and _guards_ok(a) and _guards_ok(b)


@pytest.mark.parametrize("where", ["p", "e"])
@pytest.mark.parametrize("offset", [0, 1], ids=["vector", "element-wise"])
def test_ema_kernel_keeps_elements_that_would_not_be_finite(ops, offset, where):
    n = _lengths(ops, offset)[-1] + 6  # a whole turn, a partial one and a tail
    at = [0, 1, 2, 517, n // 2, n - 3, n - 2, n - 1]
    vals = [np.inf, -np.inf, np.nan, np.nan, np.inf, -np.inf, np.nan, np.inf]
    for w in (np.float32(0.1), np.float32(0.8)):
        e, p = _pair(n, 5)
        clean = M.lerp32(e, p, w)
        (p if where == "p" else e)[at] = vals
        got_e, got_p = ops.ema_update(e, p, w, offset_floats=offset, guard=GUARD, fill=FILL)
        assert np.array_equal(_bits(got_e[0])[at], _bits(e)[at]), "a planted element did not keep e"
        rest = np.ones(n, bool)
        rest[at] = False
        assert np.array_equal(_bits(got_e[0])[rest], _bits(clean)[rest]), "a neighbour of a planted element did not update"
        assert _same(got_e[0], M.lerp32(e, p, w)) and _same(got_p[0], p) and _guards_ok(got_e) and _guards_ok(got_p)
    e, p = _pair(64, 6)  # finite operands whose difference overflows
    p[3], e[3] = np.float32(3e38), np.float32(-3e38)
    got_e, _ = ops.ema_update(e, p, np.float32(0.8), offset_floats=offset, guard=GUARD, fill=FILL)
    assert _bits(got_e[0])[3] == _bits(e)[3] and _same(got_e[0], M.lerp32(e, p, np.float32(0.8)))


@pytest.mark.parametrize("offset", [0, 1], ids=["vector", "element-wise"])
def test_exchange_kernel_swaps_words(ops, offset):
    for n in _lengths(ops, offset):
        rng = np.random.RandomState(n)
        a = rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        b = rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x7F800000, 0x00000001], np.uint32)  # NaN payloads, -0, inf, a subnormal
        a[:min(n, 6)] = special[:min(n, 6)]
        b[-min(n, 6):] = special[:min(n, 6)]
        ga, gb = ops.exchange(a, b, offset_floats=offset, guard=GUARD, fill=FILL)
        assert np.array_equal(ga[0], b) and np.array_equal(gb[0], a), "n = %d" % n
        assert all(np.all(g.view(np.float32) == FILL) and g.size == GUARD for g in ga[1:] + gb[1:])
        # as float32 arrays too, and twice is the identity
        fa, fb = ops.exchange(a.view(np.float32), b.view(np.float32), offset_floats=offset, guard=GUARD, fill=FILL)
        assert _same(fa[0], b.view(np.float32)) and _same(fb[0], a.view(np.float32))
        ta, tb = ops.exchange(fa[0], fb[0], offset_floats=offset, guard=GUARD, fill=FILL)
        assert _same(ta[0], a.view(np.float32)) and _same(tb[0], b.view(np.float32))


def test_operator_refusals(ops):
    L = ops.L
    e, p = _pair(64, 1)
    de, dp = ops.dev(e), ops.dev(p)

    def refused(rc, word):
        try:
            assert rc == -1 and word in L.mi_last_error().decode(), (rc, L.mi_last_error())
        finally:
            L.mi_clear_error()

    refused(L.mi_op_ema_update(None, dp.ptr, 64, 0.1), "NULL")
    refused(L.mi_op_ema_update(de.ptr, None, 64, 0.1), "NULL")
    refused(L.mi_op_ema_update(de.ptr + 2, dp.ptr, 8, 0.1), "4-byte aligned")
    refused(L.mi_op_ema_update(de.ptr, dp.ptr + 1, 8, 0.1), "4-byte aligned")
    for w in (-0.1, 1.5, float("nan")):
        refused(L.mi_op_ema_update(de.ptr, dp.ptr, 64, w), "w lies in [0, 1]")
    refused(L.mi_op_ema_update(de.ptr, dp.ptr, 0, 0.1), "n lies in")
    refused(L.mi_op_exchange(None, dp.ptr, 64), "NULL")
    refused(L.mi_op_exchange(de.ptr, dp.ptr + 2, 8), "4-byte aligned")
    refused(L.mi_op_exchange(de.ptr, dp.ptr, 0), "n lies in")
    refused(L.mi_op_exchange(de.ptr, de.ptr + 4 * 16, 17), "overlap")
    refused(L.mi_op_exchange(de.ptr + 4 * 16, de.ptr, 17), "overlap")
    refused(L.mi_op_exchange(de.ptr, de.ptr, 4), "overlap")
    assert _same(de.get(), e) and _same(dp.get(), p), "a refused call wrote something"
    assert L.mi_op_exchange(de.ptr, de.ptr + 4 * 16, 16) == 0  # adjacent ranges are fine
    assert _same(de.get(), np.concatenate([e[16:32], e[:16], e[32:]]))


# ---- 2. the trainer ----
def _params(dims):
    key = (dims["input"], dims["n_conv_blocks"], tuple(dims["is_block_spatial_reduction"]))
    if key not in _PARAMS:
        _PARAMS[key] = synth.make_params(dims, perturb_bn=True)
    return _PARAMS[key]


def _trainer(dims, batch, dtype=F32, track=True, params=None, **kw):
    from resnet_amd import Trainer
    from resnet_amd import binding as B
    tr = Trainer(dims, batch, **kw)
    if tr.L.mi_device_count() < 1:
        pytest.fail("no HIP device: this test must run on the MI355X box")
    tr.set_dtype(dtype)
    tr.set_params(params if params is not None else _params(dims))
    tr.source_host(B.MI_LAYOUT_NHWC)
    if track:
        tr.track_running_stats(0.1)
    return tr


def _load(tr, dims, batch, step):
    im, lab = synth.make_batch(dims, batch, step=step)
    tr.fill_host_batch(im, lab)
    tr.load_new_batch()
    return im, lab


def _step(tr, dims, batch, step):
    _load(tr, dims, batch, step)
    tr.forward()
    loss = tr.loss()
    tr.backward()
    tr.update()
    return loss


def _raw(tr):
    """what is averaged: every location, then both halves of the running arena"""
    return [tr.get("params", i) for i in range(tr.n_locations)] + list(tr.running_stats())


def _ema(tr):
    return [tr.ema_get(i) for i in range(tr.n_locations)] + list(tr.ema_running_stats())


def _assert_lists_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        bad = int(np.sum(_bits(g) != _bits(w))) if g.shape == w.shape else -1
        assert bad == 0, "%s: entry %d (locations, then running means, running vars): %d elements differ" % (what, i, bad)


VALUE_CASES = [("every1", F32, 0.9, 1, False), ("every2", F32, 0.9, 2, False), ("warmup", F32, 0.9999, 1, True), ("bf16", BF16, 0.9, 1, False)]


@pytest.mark.parametrize("case", VALUE_CASES, ids=[c[0] for c in VALUE_CASES])
def test_ema_values_follow_the_model_at_every_step(case):
    _, dtype, decay, every, warmup = case
    dims, batch = NETS["C1S"]
    tr = _trainer(dims, batch, dtype, lr=1e-3)
    try:
        tr.set_optimizer("sgd", momentum=0.9)
        tr.set_ema(decay, every=every, warmup=warmup)
        start = _raw(tr)
        _assert_lists_same(_ema(tr), start, "the snapshot")
        raws, emas, counters = [], [], []
        for step in range(5):
            _step(tr, dims, batch, step)
            raws.append(_raw(tr))
            emas.append(_ema(tr))
            counters.append(tr.ema_updates())
        assert tr.check_errors() == 0
        prev = start
        for step, cur in enumerate(raws):  # lr is large enough: every tensor and both statistics move at every step
            for i, (a, b) in enumerate(zip(prev, cur)):
                assert not np.array_equal(a, b), "step %d: entry %d did not move; the comparison would be vacuous" % (step, i)
            prev = cur
        want = M.ema_run(raws, start, decay, every=every, warmup=warmup)
        assert counters == [c for _, c in want]
        if every == 2:
            assert counters == [0, 1, 1, 2, 2]
            _assert_lists_same(emas[0], start, "step 0 of every=2")
            _assert_lists_same(emas[2], emas[1], "step 2 of every=2")
        if warmup:
            assert [float(M.weight(decay, True, k)) for k in range(2)] == [float(np.float32(0.9)), float(np.float32(1 - 2 / 11))]
        for step in range(5):
            _assert_lists_same(emas[step], want[step][0], "step %d" % step)
    finally:
        tr.close()


def test_snapshot_off_on_and_reset():
    dims, batch = NETS["C1S"]
    tr = _trainer(dims, batch, lr=1e-3)
    try:
        tr.set_optimizer("sgd", momentum=0.9)
        _step(tr, dims, batch, 0)
        tr.set_ema(0.9, every=1)
        snap = _raw(tr)
        _assert_lists_same(_ema(tr), snap, "set_ema copies the current values")
        assert tr.ema_updates() == 0
        _step(tr, dims, batch, 1)
        after1 = _ema(tr)
        _assert_lists_same(after1, M.ema_run([_raw(tr)], snap, 0.9)[0][0], "the first update")
        tr.set_ema(0.9, every=0)  # off: training goes on, the averaged values and the counter stay
        for step in (2, 3):
            _step(tr, dims, batch, step)
        _assert_lists_same(_ema(tr), after1, "every = 0 freezes the values")
        assert tr.ema_updates() == 1
        tr.set_ema(0.9, every=1)  # on again: no new snapshot, the next update continues from the frozen values
        _assert_lists_same(_ema(tr), after1, "switching on again keeps the values")
        _step(tr, dims, batch, 4)
        _assert_lists_same(_ema(tr), M.ema_run([_raw(tr)], after1, 0.9, counter=1)[0][0], "continues from the frozen values")
        assert tr.ema_updates() == 2
        tr.ema_reset()
        _assert_lists_same(_ema(tr), _raw(tr), "ema_reset takes the snapshot again")
        assert tr.ema_updates() == 0
        assert tr.check_errors() == 0
    finally:
        tr.close()


def _u8_set(dims, batch, seed=77):
    dim_in = dims["input"] + 8
    n = 2 * batch + 1
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, size=(n, dim_in, dim_in, 3)).astype(np.uint8), rng.randint(0, dims["output"], size=n).astype(np.int32), dim_in


def _state(tr):
    return [tr.get(w, i) for w in ("params", "means", "vars") for i in range(tr.n_locations)] + list(tr.running_stats())


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_training_is_untouched(case):
    """two trainers, the same parameters and batches; one averages and scores the averaged model between the steps"""
    net, dtype = case
    dims, batch = NETS[net]
    u8, u8_labels, dim_in = _u8_set(dims, batch)
    plain, ema = _trainer(dims, batch, dtype), _trainer(dims, batch, dtype)
    try:
        ema.set_ema(0.5, every=1)
        for step in range(4):
            out = []
            for tr in (plain, ema):
                _load(tr, dims, batch, step)
                tr.forward()
                fc = tr.activation("fc_output")  # from weights re-laid behind the last update (and behind the last exchange)
                if step == 3:
                    out.append((fc,))
                    continue
                loss = tr.loss()
                tr.backward()
                tr.update()
                out.append((fc, np.float32(loss[0]), np.int32(loss[1])) + tuple(_state(tr)))
            for i, (a, b) in enumerate(zip(*out)):
                assert _same(np.asarray(a), np.asarray(b)), "step %d: output %d (fc_output, loss, wrong, params, means, vars, running) differs" % (step, i)
            if step < 3:
                im, lab = synth.make_batch(dims, batch, step=10 + step)
                ema.eval_use_ema(True)
                ema.eval_forward(T.nhwc_to_nchw(im), lab)
                ema.evaluate_u8(u8, u8_labels, dim_in)
                if step == 1:
                    ema.eval_use_ema(False)
                    ema.eval_forward(T.nhwc_to_nchw(im), lab)
        assert plain.check_errors() == 0 and ema.check_errors() == 0 and ema.ema_updates() == 3
    finally:
        plain.close()
        ema.close()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_averaged_model_is_what_is_scored(ops, case):
    net, dtype = case
    dims, batch = NETS[net]
    u8, u8_labels, dim_in = _u8_set(dims, batch)
    a = _trainer(dims, batch, dtype)
    b = None
    try:
        a.set_ema(0.5, every=1)
        for step in range(3):
            _step(a, dims, batch, step)
        assert a.check_errors() == 0
        raw, avg = _raw(a), _ema(a)
        assert any(not np.array_equal(x, y) for x, y in zip(raw, avg))
        im, lab = synth.make_batch(dims, batch, step=7)
        im = T.nhwc_to_nchw(im)

        def score(tr):
            tr.eval_forward(im, lab)
            tr.check()
            return tr.activation("fc_output"), tr.activation("softmax"), tr.eval_metrics()[0]

        a.eval_use_ema(True)
        got_avg = score(a)
        got_u8 = a.evaluate_u8(u8, u8_labels, dim_in)
        _assert_lists_same(_raw(a), raw, "the arenas after the exchange back")
        _assert_lists_same(_ema(a), avg, "the averaged arenas after the exchange back")
        a.eval_use_ema(False)
        got_raw = score(a)
        for values, got, what in ((avg, got_avg, "averaged"), (raw, got_raw, "raw")):
            b = _trainer(dims, batch, dtype, params=values[:-2])
            b.set_running_stats(values[-2], values[-1])
            want = score(b)
            assert _same(got[0], want[0]), "fc_output of the %s model" % what
            assert _same(got[1], want[1]), "softmax of the %s model" % what
            assert got[2] == want[2] and np.float64(got[2]["loss_sum"]).tobytes() == np.float64(want[2]["loss_sum"]).tobytes()
            if what == "averaged":  # evaluate_u8 with the averaged model: decode + the same eval pass, the last batch ragged
                b.eval_metrics(reset=True)
                for at in range(0, len(u8_labels), batch):
                    nv = min(batch, len(u8_labels) - at)
                    b.eval_forward(ops.decode_u8(u8[at:at + nv], E.center_plan(nv, dim_in, dims["input"]), dims["input"]), u8_labels[at:at + nv])
                hand = b.eval_metrics()[1]
                assert got_u8 == hand and got_u8["rows"] == len(u8_labels) and got_u8["batches"] == 3
                assert np.float64(got_u8["loss_sum"]).tobytes() == np.float64(hand["loss_sum"]).tobytes()
            b.close()
            b = None
        assert got_avg[2] != got_raw[2] or not _same(got_avg[0], got_raw[0])
    finally:
        a.close()
        if b is not None:
            b.close()


def test_data_parallel_one_rank_bucketed_update_gives_the_same_ema():
    """a one-rank communicator (all-reduce = identity) with buckets small enough that update_parameters runs bucket by bucket: the EMA is
    launched behind the last bucket's update and holds the bits of the single-launch run"""
    dims, batch = NETS["C4I"]
    res = []
    for with_comm in (False, True):
        tr = _trainer(dims, batch)
        try:
            if with_comm:
                nbytes = tr.L.mi_dp_unique_id_bytes()
                uid = (C.c_char * nbytes)()
                assert tr.L.mi_dp_get_unique_id(uid, nbytes) == 0, tr.error()
                assert tr.L.mi_dp_init(tr.t, 0, 1, uid, nbytes) == 0, tr.error()
                tr.L.mi_dp_set_bucket_bytes(tr.t, 256 << 10)
            tr.set_ema(0.5, every=1)
            _load(tr, dims, batch, 0)
            tr.forward(); tr.backward(); tr.check()
            if with_comm:
                fr, to = (C.c_size_t * 64)(), (C.c_size_t * 64)()
                assert tr.L.mi_debug_last_buckets(tr.t, fr, to, 64) >= 2
            tr.update()
            assert tr.check_errors() == 0 and tr.ema_updates() == 1
            res.append((_raw(tr), _ema(tr)))
        finally:
            tr.close()
    _assert_lists_same(res[1][0], res[0][0], "parameters with / without buckets")
    _assert_lists_same(res[1][1], res[0][1], "EMA with / without buckets")
    assert any(not np.array_equal(x, y) for x, y in zip(*res[0]))


# ---- 3. checkpoint ----
def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_checkpoint(tmp_path, capfd):
    dims, batch = NETS["C1S"]
    listing, kept = {}, None
    for on in (True, False):
        tr = _trainer(dims, batch, dump_dir="ck")
        try:
            root = str(tmp_path / ("on" if on else "off"))
            tr.L.mi_trainer_set_dump_root(tr.t, root.encode())
            if on:
                tr.set_ema(0.9, every=1, warmup=True)
            for step in range(3):
                _step(tr, dims, batch, step)
            assert tr.check_errors() == 0
            if on:
                tr.set_ema(0.9, every=0, warmup=True)  # switched off: still dumped
                kept = _ema(tr), tr.ema_updates(), _raw(tr)
            tr.L.dump_trainer(5, tr.t, b"ck")
            tr.check()
            listing[on] = _files(root)
        finally:
            tr.close()
    base = os.path.join("ck", "%08d" % 5)
    extra = [os.path.join(base, "ema", "%03d.buffer" % i) for i in range(len(kept[0]) - 2)] + [os.path.join(base, "ema_state.buffer")]
    assert sorted(set(listing[True]) - set(listing[False])) == sorted(extra) and set(listing[False]) <= set(listing[True])
    assert not [f for f in listing[False] if "ema" in f]
    for f in listing[False]:  # averaging changes no other file of a dump
        assert open(str(tmp_path / "on" / f), "rb").read() == open(str(tmp_path / "off" / f), "rb").read(), f
    for i, want in enumerate(kept[0][:-2]):
        assert _same(np.fromfile(str(tmp_path / "on" / base / "ema" / ("%03d.buffer" % i)), np.float32), want)
    raw = open(str(tmp_path / "on" / base / "ema_state.buffer"), "rb").read()
    ch = kept[0][-1].size
    assert len(raw) == 8 + 2 * ch * 4 and np.frombuffer(raw[:8], np.int64)[0] == kept[1] == 3
    assert _same(np.frombuffer(raw[8:], np.float32), np.concatenate(kept[0][-2:]))
    capfd.readouterr()
    for src in ("on", "off"):
        tr = _trainer(dims, batch, dump_dir="ck")
        try:
            tr.L.mi_trainer_set_dump_root(tr.t, str(tmp_path / src).encode())
            tr.set_ema(0.9, every=1, warmup=True)
            _step(tr, dims, batch, 9)  # the EMA holds something else before the restore
            tr.L.overwrite_model_params(tr.t, 5, b"ck")
            tr.check()
            _assert_lists_same(_raw(tr), kept[2], "restored parameters and running statistics")
            err = capfd.readouterr().err
            if src == "on":
                _assert_lists_same(_ema(tr), kept[0], "restored averaged model")
                assert tr.ema_updates() == 3 and "averaged model" not in err
            else:  # a dump without ema/: a snapshot of what was restored, counter 0, one note
                _assert_lists_same(_ema(tr), kept[2], "snapshot of the restored values")
                assert tr.ema_updates() == 0 and err.count("no averaged model") == 1, err
        finally:
            tr.close()


# ---- 4. refusals ----
def test_trainer_refusals():
    dims, batch = NETS["C1S"]
    tr = _trainer(dims, batch, track=False)
    L, t = tr.L, tr.t

    def refused(rc, word):
        try:
            assert rc == -1 and word in tr.error(), (rc, tr.error())
        finally:
            L.mi_clear_error()

    try:
        buf = np.zeros(max(tr.sizes), np.float32)
        refused(L.mi_trainer_set_ema(t, 0.9, 1, 0), "never tracked")
        tr.track_running_stats(0.1)
        ch = L.mi_trainer_running_stats_channels(t)
        stat = np.ones(ch, np.float32)
        before = tr.device_bytes()
        refused(L.mi_trainer_eval_use_ema(t, 1), "mi_trainer_set_ema")
        refused(L.mi_trainer_ema_reset(t), "mi_trainer_set_ema")
        refused(L.mi_trainer_ema_get_location(t, 0, buf.ctypes.data), "mi_trainer_set_ema")
        refused(L.mi_trainer_ema_set_location(t, 0, buf.ctypes.data), "mi_trainer_set_ema")
        refused(L.mi_trainer_ema_get_running_stats(t, stat.ctypes.data, stat.ctypes.data), "mi_trainer_set_ema")
        refused(L.mi_trainer_ema_set_running_stats(t, stat.ctypes.data, stat.ctypes.data), "mi_trainer_set_ema")
        for decay in (1.0, -0.1, float("nan")):
            refused(L.mi_trainer_set_ema(t, decay, 1, 0), "decay lies in [0, 1)")
        refused(L.mi_trainer_set_ema(t, 0.9, -1, 0), "every")
        assert tr.device_bytes() == before and tr.ema_updates() == 0, "a refused set_ema allocated something"
        tr.set_ema(0.9, every=2)
        arena = L.mi_debug_arena_floats(tr.c_dims)
        assert tr.device_bytes() - before == 4 * (arena + 2 * ch), "the EMA arenas: the parameter arena plus 2 x channels floats"
        for decay in (1.0, -0.1, float("nan")):
            refused(L.mi_trainer_set_ema(t, decay, 1, 0), "decay lies in [0, 1)")
        refused(L.mi_trainer_set_ema(t, 0.9, -1, 0), "every")
        _step(tr, dims, batch, 0)
        _step(tr, dims, batch, 1)
        assert tr.ema_updates() == 1, "a refused set_ema changed the setting"
        held = _ema(tr)
        for i in (-1, tr.n_locations):
            refused(L.mi_trainer_ema_get_location(t, i, buf.ctypes.data), "no such location")
            refused(L.mi_trainer_ema_set_location(t, i, buf.ctypes.data), "no such location")
        for bad in (np.nan, np.inf):
            v = held[0].copy()
            v[v.size // 2] = bad
            refused(L.mi_trainer_ema_set_location(t, 0, v.ctypes.data), "not finite")
        for bad_m, bad_v, word in ((np.nan, 1.0, "not finite"), (0.0, np.inf, "not finite"), (0.0, -1e-3, "negative")):
            mm, vv = stat.copy(), stat.copy()
            mm[ch // 2], vv[ch // 3] = bad_m, bad_v
            refused(L.mi_trainer_ema_set_running_stats(t, mm.ctypes.data, vv.ctypes.data), word)
        _assert_lists_same(_ema(tr), held, "a refused call changed the averaged model")
        # the setters that are not refused do write
        tr.ema_set(1, held[1] + np.float32(1))
        tr.set_ema_running_stats(held[-2] + np.float32(1), held[-1] + np.float32(1))
        now = _ema(tr)
        assert _same(now[1], held[1] + np.float32(1)) and _same(now[-1], held[-1] + np.float32(1)) and _same(now[0], held[0])
        assert tr.check_errors() == 0
    finally:
        tr.close()


# ---- 5. memory hygiene, and a rebuild of the buffers ----
def test_red_zones_around_a_step_with_ema_and_an_ema_eval(ops):
    L = ops.L
    dims, batch = NETS["C1S_batch5"]
    assert L.mi_debug_redzone(4096, 0xFF) == 0
    try:
        tr = _trainer(dims, batch, BF16)
        try:
            tr.set_ema(0.9, every=1)
            im, lab = synth.make_batch(dims, batch, step=3)
            _step(tr, dims, batch, 0)
            tr.eval_use_ema(True)
            tr.eval_forward(T.nhwc_to_nchw(im), lab)
            tr.evaluate_u8(*_u8_set(dims, batch))
            _step(tr, dims, batch, 1)
            assert tr.check_errors() == 0 and tr.ema_updates() == 2
            assert L.mi_debug_redzone_check() == 0, tr.error()
        finally:
            tr.close()
        assert L.mi_debug_redzone_check() == 0, L.mi_last_error()
        checked, live = C.c_size_t(0), C.c_size_t(0)
        L.mi_debug_redzone_stats(C.byref(checked), None, C.byref(live))
        assert checked.value > 0
    finally:
        L.mi_debug_redzone(0, 0)


def test_the_averaged_model_survives_a_rebuild_of_the_buffers():
    from resnet_amd import binding as B
    dims, batch = NETS["C4I"]
    runs = []
    for rebuild in (False, True):
        tr = _trainer(dims, batch)
        try:
            if not rebuild:
                tr.set_store_policy(B.MI_STORE_RECOMPUTE_BN)
            tr.set_ema(0.5, every=1)
            for step in range(3):
                if rebuild and step == 2:
                    tr.set_store_policy(B.MI_STORE_RECOMPUTE_BN)  # every activation buffer dropped and rebuilt; FAST and RECOMPUTE_BN give the same bits
                _step(tr, dims, batch, step)
            assert tr.check_errors() == 0 and tr.ema_updates() == 3
            runs.append(_ema(tr))
        finally:
            tr.close()
    _assert_lists_same(runs[1], runs[0], "EMA behind a rebuild")
