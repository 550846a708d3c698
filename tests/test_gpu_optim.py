"""Momentum SGD and LARS on the GPU (kernels_optim.hip, mi_trainer_set_optimizer, mi_op_momentum_update) against the float64
model of optim_ref.py.

  operator     at the ResNet-50 arena geometry (offsets from a trainer), w / g / b with magnitudes 1e-4 .. 1e2 across tensors,
               wd 0 and 5e-5, 3 consecutive calls: w and b per tensor, the squared norms, bit-identical repeats
  guards       NaN / Inf gradients, the flag, the arena left behind, an all-zero gradient on the trust-1 path
  trainer      12 teacher-forced steps on C1S at batch 4, fp32 and bf16: the loss of the product's current parameters against
               the oracle / the bf16 model (stale re-laid weights), every update against the model fed the product's own state,
               a learning-rate change at step 6
  data parallel per-bucket LARS (one-rank RCCL, 32 MB buckets) == whole-arena LARS bit for bit, ResNet-50 at batch 2
  resume       3 steps, dump, a new trainer restores and runs 2 more == 5 uninterrupted steps bit for bit
  refusal      set_optimizer after the first update
"""
import ctypes as C

import numpy as np
import pytest

import optim_ref as R
import synth
from util import LOSS_ABS, rel_l2

pytestmark = pytest.mark.gpu

# set before measuring: the update is a handful of fp32 operations per element against float64
UPD_REL = 1e-6
UPD_MAX = 2e-6   # x max |ref| of the tensor
NORM_REL = 1e-6
MU, TAU = float(np.float32(0.9)), float(np.float32(0.001))
KINDS = {"sgd": R.SGD, "lars": R.LARS}


def _is_weight(dims):
    return [1 if kind in ("w", "fc") else 0 for _, kind, _ in synth.location_table(dims)]


def _arena_offsets(tr):
    """float offsets of locations[] in the trainer's parameter arena, then the end of the last tensor"""
    p = tr.t.contents.model.contents.params.contents
    base = C.cast(p.locations[0], C.c_void_p).value
    off = [(C.cast(p.locations[i], C.c_void_p).value - base) // 4 for i in range(p.n_locations)]
    return off + [off[-1] + tr.sizes[-1]]


def _check_update(what, got_w, got_b, ref_w, ref_b):
    """per tensor: w and b against the float64 model"""
    for i in range(len(ref_w)):
        for name, got, ref in (("w", got_w, ref_w), ("b", got_b, ref_b)):
            g, r = got[i], ref[i]
            e = rel_l2(g, r)
            m = float(np.max(np.abs(np.asarray(g, np.float64) - r)))
            scale = float(np.max(np.abs(r)))
            assert e <= UPD_REL and m <= UPD_MAX * scale, "%s: tensor %d %s: rel-L2 %.3e, max-abs %.3e (max|ref| %.3e)" % (
                what, i, name, e, m, scale)


def _split(a, offs):
    return [a[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


# ---- the operator ----
@pytest.fixture(scope="module")
def r50_geometry():
    from resnet_amd import Trainer
    tr = Trainer(synth.R50_DIMS, 1)
    if tr.L.mi_device_count() < 1:
        pytest.fail("no HIP device: this test must run on the MI355X box")
    try:
        offs = _arena_offsets(tr)
        assert all(offs[i + 1] - offs[i] == s for i, s in enumerate(tr.sizes))  # ResNet-50 has no alignment padding
    finally:
        tr.close()
    return offs, _is_weight(synth.R50_DIMS)


def _spread_state(offs, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(3):  # w, g, b
        parts = [rng.standard_normal(offs[i + 1] - offs[i], dtype=np.float32) * np.float32(10.0 ** rng.uniform(-4, 2))
                 for i in range(len(offs) - 1)]
        out.append(np.concatenate(parts))
    return out


@pytest.mark.parametrize("wd", [0.0, 5e-5])
@pytest.mark.parametrize("kind", list(KINDS))
def test_operator_per_element_at_resnet50_geometry(ops, r50_geometry, kind, wd):
    offs, is_w = r50_geometry
    lr = 0.5 if kind == "lars" else 0.01
    w, g, b = _spread_state(offs, 11 if wd else 12)
    wd32 = float(np.float32(wd))
    for call in range(3):
        if call:
            g = _spread_state(offs, 100 + call)[1]
        nw, ng, nb, flag, sq = ops.momentum_update(KINDS[kind], w, g, b, offs, is_w, lr, wd, MU, TAU)
        assert flag == 0 and not np.any(ng)
        ref_sq = R.sq_norms(_split(w, offs), _split(g, offs))
        e = np.abs(sq - ref_sq) / np.maximum(ref_sq, 1e-300)
        assert e.max() <= NORM_REL, "%s call %d: squared norm of tensor %d off by %.3e relative" % (kind, call, int(np.argmax(e) // 2), e.max())
        ref_w, _, ref_b, rflag = R.step(KINDS[kind], _split(w, offs), _split(g, offs), _split(b, offs), is_w, float(np.float32(lr)), wd32, MU, TAU)
        assert rflag == 0
        _check_update("%s wd %g call %d" % (kind, wd, call), _split(nw, offs), _split(nb, offs), ref_w, ref_b)
        if call == 0:  # the same inputs give the same bits
            w2, g2, b2, _, sq2 = ops.momentum_update(KINDS[kind], w, g, b, offs, is_w, lr, wd, MU, TAU)
            assert np.array_equal(w2, nw) and np.array_equal(b2, nb) and np.array_equal(sq2, sq) and not np.any(g2)
        w, b = nw, nb


def _small_geometry(dims):
    offs = [0]
    for size, _, _ in synth.location_table(dims):
        offs.append(offs[-1] + (size + 63) // 64 * 64)
    return offs


@pytest.mark.parametrize("kind", list(KINDS))
def test_operator_guards(ops, kind):
    """NaN in one gradient element of tensor j, Inf in tensor k < j: LARS keeps those two tensors' w and b whole, SGD (no norm pass)
    the two elements; every other tensor is updated; the flag reads j + 1; the non-finite gradients stay, all others are cleared"""
    dims = synth.C1S_DIMS
    offs, is_w = _small_geometry(dims), _is_weight(dims)
    w, g, b = _spread_state(offs, 21)
    j, k = 12, 4
    pj, pk = offs[j] + 5, offs[k] + 1
    g[pj], g[pk] = np.nan, np.inf
    nw, ng, nb, flag, _ = ops.momentum_update(KINDS[kind], w, g, b, offs, is_w, 0.1, 5e-5, MU, TAU)
    assert flag == j + 1
    assert np.isnan(ng[pj]) and np.isinf(ng[pk])
    rest = np.ones(ng.size, bool)
    rest[[pj, pk]] = False
    assert not np.any(ng[rest])
    for i in range(len(offs) - 1):
        sl = slice(offs[i], offs[i + 1])
        if i in (j, k) and kind == "lars":
            assert np.array_equal(nw[sl], w[sl]) and np.array_equal(nb[sl], b[sl]), "tensor %d changed" % i
            continue
        changed = nb[sl] != b[sl]  # (w may not move by a whole ulp where the step is small against it)
        if i in (j, k):
            p = (pj if i == j else pk) - offs[i]
            assert nw[sl][p] == w[sl][p] and nb[sl][p] == b[sl][p]
            changed[p] = True
        assert changed.all(), "tensor %d not updated" % i
    ref_w, ref_g, ref_b, rflag = R.step(KINDS[kind], _split(w, offs), _split(g, offs), _split(b, offs), is_w, float(np.float32(0.1)),
                                        float(np.float32(5e-5)), MU, TAU)
    assert rflag == flag
    _check_update(kind + " guards", _split(nw, offs), _split(nb, offs), ref_w, ref_b)


@pytest.mark.parametrize("kind", list(KINDS))
def test_operator_scalar_tail(ops, kind):
    """a tensor whose length is no multiple of 4 ends in scalar code behind the float4 body of its last chunk (the norm pass and the
    update).  Every ResNet-50 tensor is a multiple of 4 long, so the ResNet-50 geometry never runs it; a 10-class FC bias does.  Three
    tensors, the last 8192 + 7 floats (one whole chunk, then a chunk of one float4 and three scalars) -- the operator takes a tensor's
    length from the gap to the next offset, and only the last tensor's end need not be a multiple of 4.  Momentum state of the size of
    the gradient and three calls, so that mu b is as large as the step; bounds as test_operator_per_element_at_resnet50_geometry"""
    offs = [0, 64, 64 + 4096, 64 + 4096 + 8192 + 7]
    is_w = [0, 1, 1]
    lr = 0.5 if kind == "lars" else 0.01
    w, g, b = _spread_state(offs, 41)
    wd = float(np.float32(5e-5))
    for call in range(3):
        if call:
            g = _spread_state(offs, 140 + call)[1]
        nw, ng, nb, flag, sq = ops.momentum_update(KINDS[kind], w, g, b, offs, is_w, lr, wd, MU, TAU)
        assert flag == 0 and not np.any(ng)
        ref_sq = R.sq_norms(_split(w, offs), _split(g, offs))
        e = np.abs(sq - ref_sq) / np.maximum(ref_sq, 1e-300)
        assert e.max() <= NORM_REL, "%s call %d: squared norm of tensor %d off by %.3e relative" % (kind, call, int(np.argmax(e) // 2), e.max())
        ref_w, _, ref_b, rflag = R.step(KINDS[kind], _split(w, offs), _split(g, offs), _split(b, offs), is_w, float(np.float32(lr)), wd, MU, TAU)
        assert rflag == 0
        _check_update("%s scalar tail call %d" % (kind, call), _split(nw, offs), _split(nb, offs), ref_w, ref_b)
        # the three scalar elements on their own: a fault there is 3 of 8199 elements of the tensor's rel-L2
        tail = slice(offs[-1] - 3, offs[-1])
        _check_update("%s scalar tail call %d, the last three elements" % (kind, call), [nw[tail]], [nb[tail]], [ref_w[-1][-3:]], [ref_b[-1][-3:]])
        w, b = nw, nb


def test_lars_all_zero_gradient_takes_the_trust_one_path(ops):
    dims = synth.C1S_DIMS
    offs, is_w = _small_geometry(dims), _is_weight(dims)
    w, g, b = _spread_state(offs, 31)
    z = 6
    assert is_w[z]
    sl = slice(offs[z], offs[z + 1])
    g[sl] = 0
    lr, wd = float(np.float32(0.1)), float(np.float32(5e-5))
    nw, ng, nb, flag, sq = ops.momentum_update(R.LARS, w, g, b, offs, is_w, lr, wd, MU, TAU)
    assert flag == 0 and sq[z, 1] == 0 and np.all(np.isfinite(nw)) and np.all(np.isfinite(nb))
    want_b = MU * b[sl].astype(np.float64) + lr * 1.0 * wd * w[sl].astype(np.float64)  # trust 1, g = 0
    assert rel_l2(nb[sl], want_b) <= UPD_REL
    assert rel_l2(nw[sl], w[sl].astype(np.float64) - want_b) <= UPD_REL


def test_lars_loop_turns_and_an_all_zero_weight_tensor(ops):
    """the turns of the LARS passes that the ResNet-50 geometry does not isolate, and the other half of the trust-1 guard
    (optim_ref.LOOP_TURN_OFFSETS): tensor 1 is an all-zero WEIGHT tensor with a gradient (|w| = 0, |g| > 0: trust ratio 1, the tensor
    moves; test_lars_all_zero_gradient_takes_the_trust_one_path has the |g| = 0 half); tensor 2 has 65 x 8192 + 4 floats -- 66 chunks:
    lane 0 and lane 1 of optim_trust_kernel take a second turn; tensor 3 has 1024 + 256 x 4 + 4 floats: one partial chunk whose float4
    loops take two whole turns and one more quad.  Three calls; bounds as test_operator_per_element_at_resnet50_geometry"""
    offs, is_w = R.LOOP_TURN_OFFSETS, R.LOOP_TURN_IS_WEIGHT
    w, g, b = _spread_state(offs, 51)
    z = slice(offs[1], offs[2])
    w[z] = 0
    b[z] = 0
    lr, wd = 0.5, float(np.float32(5e-5))
    for call in range(3):
        if call:
            g = _spread_state(offs, 150 + call)[1]
        nw, ng, nb, flag, sq = ops.momentum_update(R.LARS, w, g, b, offs, is_w, lr, wd, MU, TAU)
        assert flag == 0 and not np.any(ng)
        if call == 0:
            assert sq[1, 0] == 0 and sq[1, 1] > 0 and np.any(nw[z]), "the all-zero weight tensor must move with trust ratio 1"
        ref_sq = R.sq_norms(_split(w, offs), _split(g, offs))
        e = np.abs(sq - ref_sq) / np.maximum(ref_sq, 1e-300)
        assert e.max() <= NORM_REL, "call %d: squared norm of tensor %d off by %.3e relative" % (call, int(np.argmax(e) // 2), e.max())
        ref_w, _, ref_b, rflag = R.step(R.LARS, _split(w, offs), _split(g, offs), _split(b, offs), is_w, float(np.float32(lr)), wd, MU, TAU)
        assert rflag == 0
        _check_update("lars loop turns call %d" % call, _split(nw, offs), _split(nb, offs), ref_w, ref_b)
        w, b = nw, nb


# ---- the trainer ----
def _trainer(dims, batch, params, kind, lr, wd, dtype=0, **kw):
    from resnet_amd import Trainer
    from resnet_amd import binding as B
    tr = Trainer(dims, batch, lr=lr, wd=wd, **kw)
    if tr.L.mi_device_count() < 1:
        pytest.fail("no HIP device: this test must run on the MI355X box")
    tr.set_dtype(dtype)
    tr.set_optimizer(kind, momentum=MU, trust=TAU)
    assert tr.optimizer() == kind
    tr.set_params(params)
    tr.source_host(B.MI_LAYOUT_NHWC)
    return tr


def _load(tr, dims, batch, step):
    im, lab = synth.make_batch(dims, batch, step=step % 2)
    tr.fill_host_batch(im, lab)
    tr.load_new_batch()
    return im, lab


def _state(tr, which):
    return [tr.get(which, i) for i in range(tr.n_locations)]


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_trainer_teacher_forced_12_steps(oracle, kind, dtype):
    import torch_ref
    from oracle.oracle_py import OracleNet
    from test_gpu_bf16 import LOSS_ABS_BF16
    dims, batch = synth.C1S_DIMS, 4
    lr0 = 0.2 if kind == "lars" else 0.01
    lrs = [lr0] * 6 + [lr0 / 4] * 6
    wd = 5e-5
    is_w = _is_weight(dims)
    tr = _trainer(dims, batch, synth.make_params(dims, perturb_bn=True), kind, lr0, wd, dtype)
    net = OracleNet(oracle, dims, batch) if dtype == 0 else None
    try:
        for step in range(12):
            if step == 6:
                tr.set_lr(lrs[step])
            params = _state(tr, "params")
            im, lab = _load(tr, dims, batch, step)
            tr.forward()
            tr.check()
            loss, _ = tr.loss()
            if dtype == 0:
                for i in range(tr.n_locations):
                    net.param(i)[:] = params[i]
                net.set_batch(im, lab)
                net.forward()
                ol, _ = net.loss()
                assert abs(loss - ol) <= LOSS_ABS * max(1.0, abs(ol)), (kind, step, loss, ol)
            else:
                emu = torch_ref.TorchNetBF16(dims, params, eps=1e-7, gates=torch_ref.gates_of(tr, dims), stem_bf16=tr.stem_dtype() == 1,
                                             stats_before_rounding=True)
                el = float(emu.forward(torch_ref.nhwc_to_nchw(im), lab).detach())
                del emu
                assert abs(loss - el) <= LOSS_ABS_BF16, (kind, step, loss, el)
            tr.backward()
            tr.check()
            grads, moms = _state(tr, "grads"), _state(tr, "means")
            assert tr.t.contents.learning_rate == np.float32(lrs[step])
            tr.update()
            assert tr.check_errors() == 0
            ref_w, _, ref_b, flag = R.step(KINDS[kind], params, grads, moms, is_w, float(np.float32(lrs[step])), float(np.float32(wd)), MU, TAU)
            assert flag == 0
            _check_update("%s %s step %d" % (kind, "bf16" if dtype else "f32", step), _state(tr, "params"), _state(tr, "means"), ref_w, ref_b)
            for i in range(tr.n_locations):
                assert not np.any(tr.get("grads", i)) and not np.any(tr.get("vars", i))
    finally:
        tr.close()
        if net is not None:
            net.close()


def test_lars_per_bucket_equals_whole_arena_resnet50():
    """the LARS twin of test_gpu_dp.py::test_rccl_one_rank_resnet50_bucket_geometry"""
    dims, batch = synth.R50_DIMS, 2
    params = synth.make_params(dims, perturb_bn=True)
    im, lab = synth.make_batch(dims, batch, step=0)
    results = []
    for with_comm in (False, True):
        tr = _trainer(dims, batch, params, "lars", 0.5, 5e-5)
        try:
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
            tr.L.mi_device_synchronize()
            grads = _state(tr, "grads")
            tr.update()
            assert tr.check_errors() == 0
            results.append((grads, _state(tr, "params"), _state(tr, "means")))
        finally:
            tr.close()
    for which, a, b in zip(("gradient", "parameter", "momentum"), results[0], results[1]):
        for i, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), "%s %d differs between per-bucket and whole-arena LARS" % (which, i)
    assert any(np.any(m) for m in results[0][2])


def test_resume_from_a_dump_equals_an_uninterrupted_run(tmp_path):
    dims, batch = synth.C1S_DIMS, 4
    params = synth.make_params(dims, perturb_bn=True)

    def run(tr, steps):
        for s in steps:
            _load(tr, dims, batch, s); tr.forward(); tr.loss(); tr.backward(); tr.update()
            assert tr.check_errors() == 0

    tr = _trainer(dims, batch, params, "lars", 0.2, 5e-5, dump_dir="resume")
    try:
        run(tr, range(5))
        want = _state(tr, "params")
    finally:
        tr.close()
    tr = _trainer(dims, batch, params, "lars", 0.2, 5e-5, dump_dir="resume")
    tr.L.mi_trainer_set_dump_root(tr.t, str(tmp_path).encode())
    try:
        run(tr, range(3))
        tr.L.dump_trainer(3, tr.t, b"resume")
        tr.check()
    finally:
        tr.close()
    from resnet_amd import Trainer
    from resnet_amd import binding as B
    tr = Trainer(dims, batch, lr=0.2, wd=5e-5, seed=99, dump_dir="resume")
    tr.L.mi_trainer_set_dump_root(tr.t, str(tmp_path).encode())
    try:
        tr.source_host(B.MI_LAYOUT_NHWC)
        tr.L.overwrite_trainer_hyperparams(tr.t, 3, b"resume")
        tr.L.overwrite_model_params(tr.t, 3, b"resume")
        tr.set_optimizer("lars", momentum=MU, trust=TAU)
        assert any(np.any(m) for m in _state(tr, "means"))  # the momentum came back with means/
        run(tr, range(3, 5))
        for i, (x, y) in enumerate(zip(_state(tr, "params"), want)):
            assert np.array_equal(x, y), "parameter %d differs after resuming (rel-L2 %.2e)" % (i, rel_l2(x, y))
    finally:
        tr.close()


def test_set_optimizer_after_the_first_update_is_refused():
    from resnet_amd import Trainer
    from resnet_amd import binding as B
    dims, batch = synth.C1S_DIMS, 4
    tr = Trainer(dims, batch)
    try:
        tr.set_params(synth.make_params(dims, perturb_bn=True))
        tr.source_host(B.MI_LAYOUT_NHWC)
        _load(tr, dims, batch, 0); tr.forward(); tr.loss(); tr.backward(); tr.update()
        assert tr.L.mi_trainer_set_optimizer(tr.t, B.MI_OPT_LARS, 0.9, 0.001) == -1
        assert "before the first update" in tr.error()
        tr.L.mi_clear_error()
        with pytest.raises(RuntimeError):
            tr.set_optimizer("sgd")
        assert tr.optimizer() == "adam"
        v1 = _state(tr, "vars")
        _load(tr, dims, batch, 1); tr.forward(); tr.loss(); tr.backward(); tr.update()
        assert tr.check_errors() == 0
        assert any(not np.array_equal(a, b) for a, b in zip(v1, _state(tr, "vars")))  # Adam's second moments still move
    finally:
        tr.close()
