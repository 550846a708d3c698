"""Gradient clipping by the global L2 norm and norm weight decay on the GPU (kernels_optim.hip: clip_norm_kernel, clip_coef_kernel,
clip_scale_kernel, optim_update_kernel<SGD>; mi_trainer_set_clip_grad_norm, mi_trainer_set_norm_weight_decay) against the float64 model of
clipref.py, which tests/test_clip_model.py pins against torch on the CPU.

  operator     every loop turn of the three kernels on clipref.op_gradient(): squared norm to 1e-12 relative (the float64 sums run in
               another order), coefficient to one float32 ulp, every element g * coef_device bit for bit; the unclipped, all-zero, Inf /
               NaN and near-overflow cases; bit-identical repeats; the red zones
  trainer      6 teacher-forced steps on C1S at batch 4 per optimizer, clipping for four of them: every update against the model's clip
               followed by the optimizer's model, with the bounds the optimizer tests use; the record's counters
  off          set_clip_grad_norm(0): parameters, moments, device bytes and a dump byte for byte those of a trainer that never called it
  accumulation k = 3: the collecting calls leave the record alone, call 3 clips the folded gradient
  data parallel one-rank RCCL, ResNet-50 at batch 2, 32 MB buckets: clipping behind the buckets == clipping without a communicator
  norm wd      the SGD operator and trainer against the two-group model; refused under Adam and LARS
"""
import ctypes as C
import os

import numpy as np
import pytest

import accumref
import clipref as M
import ewref as E
import optim_ref as R
import synth
from test_gpu_optim import MU, TAU, _arena_offsets, _check_update, _is_weight, _split, _state

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
ZONE = 256 * 1024
WD = float(np.float32(5e-5))
ADAM_HP = dict(lr=1e-3, wd=1e-4, b1=0.9, b2=0.999, eps=1e-7)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rel(a, b):
    return abs(a - b) / abs(b)


def _check_record(rec, want, what):
    """sq_norm / norm to 1e-12 relative, coef to one float32 ulp, the flags"""
    if want["sq_norm"] > 0:
        assert _rel(rec["sq_norm"], want["sq_norm"]) <= M.OP_SQ_REL, "%s: sq_norm %.17g, model %.17g" % (what, rec["sq_norm"], want["sq_norm"])
        assert _rel(rec["norm"], want["norm"]) <= M.OP_SQ_REL, what
    else:
        assert rec["sq_norm"] == 0 and rec["norm"] == 0, what
    assert M.ulps32(rec["coef"], want["coef"]) <= 1, "%s: coef %.9g, model %.9g" % (what, rec["coef"], want["coef"])
    assert rec["nonfinite"] == want["nonfinite"], what


# ---- the operator ----
@pytest.fixture(scope="module")
def op_case():
    """the gradient of every operator case and the model's record of it (computed once)"""
    g = M.op_gradient()
    _, rec = M.clip(M.split(g, M.OP_OFFSETS), 1.0)
    return g, rec


def test_operator_clips_every_loop_turn(ops, op_case):
    """(a) max_norm half the norm: the record against the model; every element is float32(g) * coef_device bit for bit -- whole chunks, the
    partial chunk of three float4 turns, the scalar tail, 71 partials -- and a second call on the same input gives the same bits"""
    g, clean = op_case
    max_norm = float(np.float32(0.5 * clean["norm"]))
    _, want = M.clip(M.split(g, M.OP_OFFSETS), max_norm)
    got, rec = ops.clip_grad_norm(g, M.OP_OFFSETS, max_norm)
    print("sq_norm %.17g (model %.17g), coef %.9g (model %.9g)" % (rec["sq_norm"], want["sq_norm"], rec["coef"], want["coef"]))
    _check_record(rec, want, "half the norm")
    assert rec["coef"] < 1 and rec["updates"] == 1 and rec["clipped"] == 1
    expect = M.scale(g, rec["coef"])
    bad = np.flatnonzero(_bits(got) != _bits(expect))
    assert bad.size == 0, "%d elements are not g * coef, the first at %d" % (bad.size, bad[0])
    got2, rec2 = ops.clip_grad_norm(g, M.OP_OFFSETS, max_norm)
    assert rec2 == rec and np.array_equal(_bits(got2), _bits(got))


def test_operator_leaves_an_unclipped_gradient_word_for_word(ops, op_case):
    """(b) max_norm twice the norm: coef == 1, clipped stays 0, every word as it was -- a -0 and a denormal among them"""
    g, clean = op_case
    g = g.copy()
    g[5], g[M.OP_OFFSETS[2] + 9000], g[-1] = -0.0, np.float32(1e-40), np.float32(-1e-41)
    max_norm = float(np.float32(2.0 * clean["norm"]))
    got, rec = ops.clip_grad_norm(g, M.OP_OFFSETS, max_norm)
    _check_record(rec, M.clip(M.split(g, M.OP_OFFSETS), max_norm)[1], "twice the norm")
    assert rec["coef"] == 1.0 and rec["nonfinite"] == 0 and rec["updates"] == 1 and rec["clipped"] == 0
    assert np.array_equal(_bits(got), _bits(g))


def test_operator_all_zero_gradient(ops):
    """(c) norm 0: max_norm / 1e-6 is clamped to 1"""
    g = np.zeros(M.OP_OFFSETS[-1], np.float32)
    got, rec = ops.clip_grad_norm(g, M.OP_OFFSETS, 1e-3)
    assert rec["coef"] == 1.0 and rec["sq_norm"] == 0 and rec["norm"] == 0 and rec["nonfinite"] == 0 and rec["clipped"] == 0
    assert not np.any(_bits(got))


@pytest.mark.parametrize("word", [0x7F800000, 0xFF800000, 0x7FC12345], ids=["inf", "-inf", "nan"])
@pytest.mark.parametrize("where", ["whole-chunk", "float4-loop", "scalar-tail"])
def test_operator_leaves_a_gradient_that_is_not_finite(ops, op_case, word, where):
    """(d) one Inf / NaN element: nonfinite 1, coef 1, the gradient word for word (the optimizers' guards report it)"""
    g, clean = op_case
    g = g.copy()
    at = {"whole-chunk": M.OP_OFFSETS[2] + 3 * M.CHUNK + 4 * 1800 + 1, "float4-loop": M.OP_OFFSETS[3] + 4 * 300 + 2, "scalar-tail": g.size - 2}[where]
    _bits(g)[at] = word
    got, rec = ops.clip_grad_norm(g, M.OP_OFFSETS, float(np.float32(0.5 * clean["norm"])))
    assert rec["nonfinite"] == 1 and rec["coef"] == 1.0 and rec["clipped"] == 0 and rec["updates"] == 1 and not np.isfinite(rec["sq_norm"])
    assert np.array_equal(_bits(got), _bits(g))


def test_operator_squares_that_overflow_float(ops, op_case):
    """(e) elements near 1e30: sum g^2 overflows float32 and not float64; the coefficient is the model's, not 0"""
    g = op_case[0].copy()
    sl = slice(M.OP_OFFSETS[3], M.OP_OFFSETS[4])
    g[sl] = np.float32(1e30) * np.sign(g[sl])
    _, want = M.clip(M.split(g, M.OP_OFFSETS), 1.0)
    assert want["sq_norm"] > 3.5e38 and want["coef"] > 0 and want["nonfinite"] == 0
    got, rec = ops.clip_grad_norm(g, M.OP_OFFSETS, 1.0)
    _check_record(rec, want, "1e30")
    assert rec["coef"] > 0 and rec["clipped"] == 1
    assert np.array_equal(_bits(got), _bits(M.scale(g, rec["coef"])))


def test_operator_stays_inside_its_allocations(ops, op_case):
    """case (a) under the red-zone mode of the allocator: the gradient, the chunk table, the partials and the record each between two
    zones of 0xFF bytes, none of which changes; the values are those of the run without zones"""
    g, clean = op_case
    L = ops.L
    max_norm = float(np.float32(0.5 * clean["norm"]))
    plain, rec0 = ops.clip_grad_norm(g, M.OP_OFFSETS, max_norm)
    assert L.mi_debug_redzone(ZONE, 0xFF) == 0
    try:
        got, rec = ops.clip_grad_norm(g, M.OP_OFFSETS, max_norm)
        assert L.mi_debug_redzone_check() == 0, L.mi_last_error().decode()
        checked = C.c_size_t()
        L.mi_debug_redzone_stats(C.byref(checked), None, None)
        assert checked.value >= 4  # verified when they were freed
    finally:
        assert L.mi_debug_redzone(0, 0) == 0
    assert rec == rec0 and np.array_equal(_bits(got), _bits(plain))


# ---- the trainer ----
def _trainer(dims, batch, kind, dtype=F32, wd=WD, lr=None, **kw):
    from resnet_amd import Trainer
    from resnet_amd import binding as B
    if kind == "adam":
        tr = Trainer(dims, batch, **dict(ADAM_HP, **kw))
    else:
        tr = Trainer(dims, batch, lr=lr if lr is not None else (0.2 if kind == "lars" else 0.01), wd=wd, **kw)
    if tr.L.mi_device_count() < 1:
        pytest.fail("no HIP device: this test must run on the MI355X box")
    tr.set_dtype(dtype)
    if kind != "adam":
        tr.set_optimizer(kind, momentum=MU, trust=TAU)
    tr.set_params(synth.make_params(dims, perturb_bn=True))
    tr.source_host(B.MI_LAYOUT_NHWC)
    return tr


def _fwd_bwd(tr, dims, batch, step):
    im, lab = synth.make_batch(dims, batch, step=step % 2)
    tr.fill_host_batch(im, lab)
    tr.load_new_batch()
    tr.forward()
    tr.loss()
    tr.backward()
    tr.check()


_NORM0 = {}


def _first_norm(dtype):
    """the gradient norm of step 0 (a throw-away trainer: the setter is refused between forward_pass and update_parameters)"""
    if dtype not in _NORM0:
        dims, batch = synth.C1S_DIMS, 4
        tr = _trainer(dims, batch, "sgd", dtype)
        try:
            _fwd_bwd(tr, dims, batch, 0)
            _NORM0[dtype] = M.clip(_state(tr, "grads"), 1.0)[1]["norm"]
        finally:
            tr.close()
    return _NORM0[dtype]


def _expected_update(tr, kind, params, scaled, moms, vars_, is_w, wd_norm=None):
    """the optimizer's model on the clipped gradient, checked against the trainer's state"""
    t = tr.t.contents
    if kind == "adam":
        cat = lambda xs: np.concatenate([np.asarray(x, np.float32).ravel() for x in xs])
        # update_parameters advanced the decays before use: cur_* now hold the products the kernel was handed
        hp = dict(ADAM_HP, cb1=float(t.cur_mean_decay), cb2=float(t.cur_var_decay))
        bad, worst = E.adam_violations((cat(_state(tr, "params")), cat(_state(tr, "means")), cat(_state(tr, "vars"))),
                                       (cat(params), cat(scaled), cat(moms), cat(vars_)), hp)
        assert bad == 0, "Adam on the clipped gradient: %d values out of bounds (worst %.3g x 2^-24 A)" % (bad, worst)
        return
    lr, wd = float(t.learning_rate), float(t.weight_decay)
    if wd_norm is not None:
        ref_w, _, ref_b, flag = M.sgd_two_groups(params, scaled, moms, is_w, lr, wd, float(np.float32(wd_norm)), MU)
    else:
        ref_w, _, ref_b, flag = R.step(R.SGD if kind == "sgd" else R.LARS, params, scaled, moms, is_w, lr, wd, MU, TAU)
    assert flag == 0
    _check_update(kind, _state(tr, "params"), _state(tr, "means"), ref_w, ref_b)


@pytest.mark.parametrize("kind,dtype", [("adam", F32), ("sgd", F32), ("lars", F32), ("lars", BF16)], ids=["adam-f32", "sgd-f32", "lars-f32", "lars-bf16"])
def test_trainer_teacher_forced_6_steps(kind, dtype):
    """max_norm half the first step's own norm for four steps, far above any norm for the last two; the gradients are read before every
    update and the update is the model's clip followed by the optimizer's model (the LARS trust ratio taken on the clipped gradient)"""
    dims, batch = synth.C1S_DIMS, 4
    norm0 = _first_norm(dtype)
    limits = [float(np.float32(0.5 * norm0))] * 4 + [float(np.float32(1e3 * norm0))] * 2
    is_w = _is_weight(dims)
    tr = _trainer(dims, batch, kind, dtype)
    try:
        clipped = 0
        for step, max_norm in enumerate(limits):
            tr.set_clip_grad_norm(max_norm)
            _fwd_bwd(tr, dims, batch, step)
            params, grads, moms, vars_ = (_state(tr, w) for w in ("params", "grads", "means", "vars"))
            scaled, want = M.clip(grads, max_norm)
            if step == 0:
                assert _rel(want["norm"], norm0) <= 1e-12 and want["clipped"] == 1
            if step >= 4:
                assert want["clipped"] == 0
            clipped += want["clipped"]
            tr.update()
            assert tr.check_errors() == 0
            rec = tr.last_clip()
            _check_record(rec, want, "%s step %d" % (kind, step))
            assert rec["updates"] == step + 1 and rec["clipped"] == clipped, (step, rec, clipped)
            _expected_update(tr, kind, params, scaled, moms, vars_, is_w)
            assert not any(np.any(g) for g in _state(tr, "grads"))
        assert rec["coef"] == 1.0 and 1 <= clipped <= 4
    finally:
        tr.close()


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_off_means_off(tmp_path, kind):
    """set_clip_grad_norm(0) and the default wd_norm: three steps give the parameters, the moments, the device bytes and a dump of a trainer
    that never called the setter, byte for byte"""
    from resnet_amd import binding as B
    dims, batch = synth.C1S_DIMS, 4
    runs = []
    for name in ("never", "zero"):
        tr = _trainer(dims, batch, kind, dump_dir="off")
        try:
            root = str(tmp_path / name)
            tr.L.mi_trainer_set_dump_root(tr.t, root.encode())
            if name == "zero":
                tr.set_clip_grad_norm(0)
                assert tr.L.mi_trainer_last_clip(tr.t, C.byref(B.MiClipRecord())) == -1  # nothing was built
                tr.L.mi_clear_error()
            for step in range(3):
                _fwd_bwd(tr, dims, batch, step)
                tr.update()
            assert tr.check_errors() == 0
            tr.L.dump_trainer(3, tr.t, b"off")
            tr.check()
            runs.append(([_state(tr, w) for w in ("params", "means", "vars")], tr.device_bytes(), root))
        finally:
            tr.close()
    for a, b in zip(runs[0][0], runs[1][0]):
        for x, y in zip(a, b):
            assert np.array_equal(_bits(x), _bits(y))
    assert runs[0][1] == runs[1][1]
    files = _files(runs[0][2])
    assert files and files == _files(runs[1][2])
    for f in files:
        assert open(os.path.join(runs[0][2], f), "rb").read() == open(os.path.join(runs[1][2], f), "rb").read(), f


def test_accumulation_window_clips_the_folded_gradient_once():
    """k = 3, scale 1 / 3: calls 1 and 2 leave the record's counters alone; call 3 clips (acc + g) * scale, read before the call"""
    dims, batch, k = synth.C1S_DIMS, 4, 3
    scale = np.float32(1.0) / np.float32(3.0)
    is_w = _is_weight(dims)
    max_norm = float(np.float32(0.25 * _first_norm(F32)))
    tr = _trainer(dims, batch, "sgd")
    try:
        offs = _arena_offsets(tr)
        tr.set_accumulation(k, float(scale))
        tr.set_clip_grad_norm(max_norm)
        assert tr.last_clip()["updates"] == 0
        for call in range(k - 1):
            _fwd_bwd(tr, dims, batch, call)
            tr.update()
            assert tr.last_clip() == dict(sq_norm=0.0, norm=0.0, coef=0.0, nonfinite=0, updates=0, clipped=0)
        _fwd_bwd(tr, dims, batch, k - 1)
        acc = tr._to_host(C.c_void_p(tr.L.mi_debug_accum_arena(tr.t)), offs[-1])
        params, grads, moms = (_state(tr, w) for w in ("params", "grads", "means"))
        folded = [accumref.fold(acc[offs[i]:offs[i] + g.size], g, scale) for i, g in enumerate(grads)]
        scaled, want = M.clip(folded, max_norm)
        assert want["clipped"] == 1
        tr.update()
        assert tr.check_errors() == 0 and tr.accumulation() == (k, 0)
        rec = tr.last_clip()
        _check_record(rec, want, "the folded gradient")
        assert rec["updates"] == 1 and rec["clipped"] == 1
        _expected_update(tr, "sgd", params, scaled, moms, None, is_w)
    finally:
        tr.close()


@pytest.mark.parametrize("kind", ["lars", "adam"])
def test_data_parallel_clips_behind_every_bucket_resnet50(kind):
    """the form of test_gpu_optim.py::test_lars_per_bucket_equals_whole_arena_resnet50 with clipping on in both runs: the norm is that of the
    whole all-reduced gradient, so the run with a one-rank communicator and at least 3 buckets equals the run without one bit for bit"""
    dims, batch = synth.R50_DIMS, 2
    im, lab = synth.make_batch(dims, batch, step=0)
    results = []
    for with_comm in (False, True):
        tr = _trainer(dims, batch, kind, lr=0.5 if kind == "lars" else None)
        try:
            tr.set_clip_grad_norm(1e-2)
            if with_comm:
                nbytes = tr.L.mi_dp_unique_id_bytes()
                uid = (C.c_char * nbytes)()
                assert tr.L.mi_dp_get_unique_id(uid, nbytes) == 0, tr.error()
                assert tr.L.mi_dp_init(tr.t, 0, 1, uid, nbytes) == 0, tr.error()
                tr.L.mi_dp_set_bucket_bytes(tr.t, 32 << 20)
            tr.fill_host_batch(im, lab); tr.load_new_batch(); tr.forward(); tr.backward(); tr.check()
            if with_comm:
                fr, to = (C.c_size_t * 64)(), (C.c_size_t * 64)()
                assert tr.L.mi_debug_last_buckets(tr.t, fr, to, 64) >= 3
            tr.update()
            assert tr.check_errors() == 0
            rec = tr.last_clip()
            assert rec["coef"] < 1 and rec["clipped"] == 1 and rec["updates"] == 1
            results.append((rec, _state(tr, "params"), _state(tr, "means")))
        finally:
            tr.close()
    assert results[0][0] == results[1][0], "the record differs: %r, %r" % (results[0][0], results[1][0])
    for which, a, b in zip(("parameter", "momentum"), results[0][1:], results[1][1:]):
        for i, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), "%s %d differs between clipping behind the buckets and without a communicator" % (which, i)
    assert any(np.any(m) for m in results[0][2])


# ---- norm weight decay ----
NWD_IS_WEIGHT = [0, 1, 0, 1]   # the 66-chunk tensor is a gamma here: whole chunks and a chunk of one float4 pick wd_norm


def _nwd_state(seed):
    """w, g, b of one magnitude per tensor, so that a decay of 5e-5 shows far above the bounds of the update"""
    rng = np.random.default_rng(seed)
    return [np.concatenate([rng.standard_normal(n, dtype=np.float32) for n in R.LOOP_TURN_SIZES]) for _ in range(3)]


@pytest.mark.parametrize("wd_norm", [0.0, 1e-3])
def test_operator_norm_weight_decay(ops, wd_norm):
    offs = R.LOOP_TURN_OFFSETS
    w, g, b = _nwd_state(61)
    wdn = float(np.float32(wd_norm))
    for call in range(3):
        if call:
            g = _nwd_state(160 + call)[1]
        nw, ng, nb, flag, _ = ops.momentum_update(R.SGD, w, g, b, offs, NWD_IS_WEIGHT, 0.01, WD, MU, TAU, wd_norm=wd_norm)
        assert flag == 0 and not np.any(ng)
        ref_w, _, ref_b, rflag = M.sgd_two_groups(_split(w, offs), _split(g, offs), _split(b, offs), NWD_IS_WEIGHT, float(np.float32(0.01)), WD, wdn, MU)
        assert rflag == 0
        _check_update("sgd wd_norm %g call %d" % (wd_norm, call), _split(nw, offs), _split(nb, offs), ref_w, ref_b)
        # the one-group rule is far outside those bounds on the gammas, so the check above is one of the second group
        one_b = R.step(R.SGD, _split(w, offs), _split(g, offs), _split(b, offs), NWD_IS_WEIGHT, float(np.float32(0.01)), WD, MU)[2]
        for i, f in enumerate(NWD_IS_WEIGHT):
            if not f:
                assert np.linalg.norm(one_b[i] - ref_b[i]) > 10 * 1e-6 * np.linalg.norm(ref_b[i])
        w, b = nw, nb


def test_operator_norm_weight_decay_defaults(ops):
    """wd_norm == wd gives the bits of mi_op_momentum_update, and LARS ignores wd_norm"""
    offs = R.LOOP_TURN_OFFSETS
    w, g, b = _nwd_state(62)
    for kind, wd_norm in ((R.SGD, WD), (R.LARS, 0.5)):
        a = ops.momentum_update(kind, w, g, b, offs, NWD_IS_WEIGHT, 0.01, WD, MU, TAU)
        c = ops.momentum_update(kind, w, g, b, offs, NWD_IS_WEIGHT, 0.01, WD, MU, TAU, wd_norm=wd_norm)
        assert np.array_equal(_bits(a[0]), _bits(c[0])) and np.array_equal(_bits(a[2]), _bits(c[2])) and a[3] == c[3] == 0


def test_trainer_norm_weight_decay_4_sgd_steps():
    """gamma / beta follow wd_norm = 0, the weights wd = 5e-3; at step 2 wd_norm changes (it is read at every update)"""
    dims, batch = synth.C1S_DIMS, 4
    is_w = _is_weight(dims)
    tr = _trainer(dims, batch, "sgd", wd=float(np.float32(5e-3)))
    try:
        seen = 0.0
        for step, wd_norm in enumerate([0.0, 0.0, 1e-2, 1e-2]):
            tr.set_norm_weight_decay(wd_norm)
            _fwd_bwd(tr, dims, batch, step)
            params, grads, moms = (_state(tr, w) for w in ("params", "grads", "means"))
            tr.update()
            assert tr.check_errors() == 0
            _expected_update(tr, "sgd", params, [g.copy() for g in grads], moms, None, is_w, wd_norm=wd_norm)
            t = tr.t.contents
            one_b = R.step(R.SGD, params, grads, moms, is_w, float(t.learning_rate), float(t.weight_decay), MU)[2]
            got_b = _state(tr, "means")
            seen = max(seen, max(np.linalg.norm(one_b[i] - got_b[i]) / np.linalg.norm(got_b[i]) for i, f in enumerate(is_w) if not f))
        assert seen > 10 * 1e-6, "no gamma / beta tells the two-group rule from the one-group rule: %.3g" % seen
    finally:
        tr.close()


@pytest.mark.parametrize("kind", ["adam", "lars"])
def test_norm_weight_decay_is_refused_under_adam_and_lars(kind):
    dims, batch = synth.C1S_DIMS, 4
    is_w = _is_weight(dims)
    tr = _trainer(dims, batch, kind)
    try:
        assert tr.L.mi_trainer_set_norm_weight_decay(tr.t, 0.0) == -1 and "MI_OPT_SGD only" in tr.error()
        tr.L.mi_clear_error()
        with pytest.raises(RuntimeError, match="MI_OPT_SGD only"):
            tr.set_norm_weight_decay(0.0)
        _fwd_bwd(tr, dims, batch, 0)
        params, grads, moms, vars_ = (_state(tr, w) for w in ("params", "grads", "means", "vars"))
        tr.update()
        assert tr.check_errors() == 0
        _expected_update(tr, kind, params, grads, moms, vars_, is_w)  # the rule it always had
    finally:
        tr.close()


# ---- refusals ----
def test_trainer_refusals():
    dims, batch = synth.C1S_DIMS, 4
    tr = _trainer(dims, batch, "sgd")
    L, t = tr.L, tr.t
    from resnet_amd import binding as B

    def refused(rc, text):
        assert rc == -1 and text in tr.error(), (rc, tr.error())
        L.mi_clear_error()

    try:
        before = tr.device_bytes()
        rec = B.MiClipRecord()
        refused(L.mi_trainer_last_clip(t, C.byref(rec)), "never on")
        for bad in (float("nan"), float("inf"), -1.0):
            refused(L.mi_trainer_set_clip_grad_norm(t, bad), "finite and >= 0")
            refused(L.mi_trainer_set_norm_weight_decay(t, bad), "finite and >= 0")
        assert tr.device_bytes() == before, "a refused call allocated something"
        tr.set_clip_grad_norm(2.5)
        grown = tr.device_bytes() - before
        chunks = sum(len(R.chunks_of(n)) for n in tr.sizes)
        assert grown == chunks * (16 + 8) + C.sizeof(B.MiClipRecord)
        tr.set_clip_grad_norm(0)
        tr.set_clip_grad_norm(1.5)  # as often as one likes, one table
        assert tr.device_bytes() - before == grown
        refused(L.mi_trainer_last_clip(t, None), "NULL")
        im, lab = synth.make_batch(dims, batch, step=0)
        tr.fill_host_batch(im, lab); tr.load_new_batch(); tr.forward()
        refused(L.mi_trainer_set_clip_grad_norm(t, 1.0), "between forward_pass and update_parameters")
        tr.loss(); tr.backward()
        refused(L.mi_trainer_set_clip_grad_norm(t, 0.0), "between forward_pass and update_parameters")
        tr.update()
        assert tr.check_errors() == 0 and tr.last_clip()["updates"] == 1
        tr.set_accumulation(2, 0.5)
        _fwd_bwd(tr, dims, batch, 1)
        tr.update()
        assert tr.accumulation() == (2, 1)
        refused(L.mi_trainer_set_clip_grad_norm(t, 1.0), "pending")
        with pytest.raises(RuntimeError, match="pending"):
            tr.set_clip_grad_norm(0)
        _fwd_bwd(tr, dims, batch, 2)
        tr.update()
        assert tr.check_errors() == 0 and tr.last_clip()["updates"] == 2
        tr.set_clip_grad_norm(0)  # between windows
    finally:
        tr.close()
