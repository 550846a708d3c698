"""Mixing in the trainer (mi_trainer_set_mix / mi_trainer_last_mix, include/resnet_mi.h "mixing") on C1S at batch 5 and 8, synthetic source,
and on uint8 shards.

  images          after load_new_batch = the numpy mix (tests/mixref.py) of an unmixed twin's images under last_mix(), bit for bit;
                  output_layer_deriv = the float32 two-label model on the trainer's own pred
  linearity       the mixed step's parameter gradients = lam g_a + (1 - lam) g_b of two one-label steps on the mixed images
  three steps     LARS, smoothing 0.1, mixing on: clean, finite
  uint8 shards    prefetch on and off: the same pixels and plans over a shard boundary and an epoch change; dump and resume
  refusals, and no mix launch anywhere while mixing was never enabled
"""
import ctypes as C

import numpy as np
import pytest

import lossref
import mixref as R
import synth

pytestmark = pytest.mark.gpu

DIMS = synth.C1S_DIMS
L_OUT = DIMS["output"]
MIX = dict(mixup=0.8, cutmix=1.0, prob=1.0, switch=0.5)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _plan(seed, epoch, step, dim, rank=0, world=1, **kw):
    s = dict(MIX, **kw)
    return R.plan(seed, epoch, step, rank, world, s["mixup"], s["cutmix"], s["prob"], s["switch"], dim)


def _seed_with_both_modes(steps, dim):
    """the first seed whose plans at the given steps hold a mixup and a CutMix draw with a box that is not empty"""
    for seed in range(1000):
        ps = [_plan(seed, 0, s, dim) for s in steps]
        if {p["mode"] for p in ps} == {1, 2} and all(p["mode"] == 1 or (p["y1"] > p["y0"] and p["x1"] > p["x0"]) for p in ps):
            return seed
    raise AssertionError("no such seed")


@pytest.fixture(scope="module")
def params():
    return synth.make_params(DIMS, perturb_bn=True)


def _trainer(params, batch, smoothing=0.0, device=True):
    from resnet_amd import Trainer
    tr = Trainer(DIMS, batch)
    if tr.L.mi_device_count() < 1:
        pytest.fail("no HIP device: this test must run on the MI355X box")
    tr.set_params(params)
    if device:
        tr.set_loss(smoothing=smoothing, topk=5, device=True)
    return tr


def _same_plan(got, want):
    return all(got[k] == want[k] for k in ("mode", "y0", "x0", "y1", "x1")) and np.float32(got["lam"]).tobytes() == np.float32(want["lam"]).tobytes()


@pytest.mark.parametrize("batch", [5, 8])
def test_images_and_head_after_load(params, batch):
    steps = 3
    seed = _seed_with_both_modes(range(-1, steps - 1), DIMS["input"])
    eps = 0.1
    mixed, twin = _trainer(params, batch, eps), _trainer(params, batch, eps)
    try:
        mixed.set_mix(seed=seed, **MIX)
        for tr in (mixed, twin):
            tr.source_synthetic(pool_batches=steps)
        for step in range(steps):
            mixed.load_new_batch()
            twin.load_new_batch()
            p = mixed.last_mix()
            assert _same_plan(p, _plan(seed, 0, step - 1, DIMS["input"])), (step, p)  # cur_dump_id before its increment: -1 at the first load
            plain = twin.activation("input")
            got = mixed.activation("input")
            assert _same(got, R.mix(plain, p)), "step %d, mode %d" % (step, p["mode"])
            assert not _same(got, plain)
            lab = mixed.labels()
            assert np.array_equal(lab, twin.labels())
            mixed.forward()
            mixed.check()
            pred = mixed.activation("softmax")
            want = pred - R.targets_f32(L_OUT, lab, R.labels_b(lab), p["lam"], eps)
            assert _same(mixed.activation("fc_output", deriv=True), want), "step %d: output_layer_deriv" % step
            last, _ = mixed.metrics()
            assert last["rows"] == batch and np.isfinite(last["loss_sum"])
            assert last["wrong_top1"] == int(np.sum(lossref.rank_of(pred, lab) >= 1))
            mixed.backward()
            mixed.update()
            assert mixed.check_errors() == 0
    finally:
        mixed.close()
        twin.close()


@pytest.mark.parametrize("mode", ["mixup", "cutmix"])
@pytest.mark.parametrize("batch", [5, 8])
def test_gradients_are_linear_in_the_two_labels(params, batch, mode):
    """one backward of the mixed batch with both labels = lam x (the backward with labels a) + (1 - lam) x (the backward with labels b) on the
    same mixed pixels: the forward passes are the same launches on the same bits, and the backward pass is linear in dlogits.  Allowed: the
    relative L2 tests/test_gpu_net.py grants a parameter gradient"""
    from resnet_amd import binding as B
    from test_gpu_net import PARAM_REL_L2
    eps = 0.1
    kw = dict(mixup=0.8, cutmix=0.0) if mode == "mixup" else dict(mixup=0.0, cutmix=1.0)
    seed = next(s for s in range(1000) if (lambda p: p["mode"] != 2 or (p["y1"] - p["y0"]) * (p["x1"] - p["x0"]) > 16)(_plan(s, 0, -1, DIMS["input"], **kw)))
    mixed = _trainer(params, batch, eps)
    singles = [_trainer(params, batch, eps) for _ in range(2)]
    try:
        mixed.set_mix(seed=seed, prob=1.0, switch=0.5, **kw)
        mixed.source_synthetic()
        mixed.load_new_batch()
        p = mixed.last_mix()
        lam = float(p["lam"])
        assert p["mode"] == (1 if mode == "mixup" else 2) and 0.0 < lam < 1.0
        images, lab = mixed.activation("input"), mixed.labels()
        mixed.forward()
        mixed.backward()
        mixed.check()
        g = [mixed.get("grads", i).astype(np.float64) for i in range(mixed.n_locations)]
        parts = []
        for tr, labels in zip(singles, (lab, R.labels_b(lab))):
            tr.source_host(B.MI_LAYOUT_NCHW)
            tr.fill_host_batch(images, labels)
            tr.load_new_batch()
            assert _same(tr.activation("input"), images)
            tr.forward()
            tr.backward()
            tr.check()
            parts.append([tr.get("grads", i).astype(np.float64) for i in range(tr.n_locations)])
        worst = 0.0
        for i, (gm, ga, gb) in enumerate(zip(g, *parts)):
            want = lam * ga + (1.0 - lam) * gb
            rel = float(np.linalg.norm(gm - want) / (np.linalg.norm(want) + 1e-30))
            worst = max(worst, rel)
            assert rel <= PARAM_REL_L2, "tensor %d: rel-L2 %.3e" % (i, rel)
        print("%s batch %d lam %.4f: worst rel-L2 of a parameter gradient %.3e" % (mode, batch, lam, worst))
    finally:
        mixed.close()
        for tr in singles:
            tr.close()


def test_three_full_steps_with_lars_and_smoothing(params):
    tr = _trainer(params, 8, 0.1)
    try:
        tr.set_optimizer("lars")
        tr.set_mix(seed=_seed_with_both_modes(range(-1, 2), DIMS["input"]), **MIX)
        tr.source_synthetic()
        modes = []
        for _ in range(3):
            tr.load_new_batch()
            tr.forward()
            last, _ = tr.metrics()
            assert np.isfinite(last["loss_sum"]) and last["loss_sum"] > 0 and last["rows"] == 8
            tr.backward()
            tr.update()
            assert tr.check_errors() == 0
            modes.append(tr.last_mix()["mode"])
        tr.check()
        assert set(modes) == {1, 2}
        assert all(np.all(np.isfinite(tr.get("params", i))) for i in range(tr.n_locations))
    finally:
        tr.close()


# ---------------------------------------------------------------- uint8 shards
DIN, DOUT, AUG_SEED, MIX_SEED = 40, 32, 4242, 7


def _u8_trainer(u8, per_shard, batch, prefetch, root=None, **kw):
    from test_gpu_input_u8 import make_trainer
    tr = make_trainer(batch, per_shard, **kw)
    if root:
        tr.L.mi_trainer_set_dump_root(tr.t, root.encode())
    tr.source_shards_u8(u8, DIN, augment="random", flip=True, seed=AUG_SEED, prefetch=prefetch)
    tr.set_loss(smoothing=0.1, topk=5, device=True)
    tr.set_mix(seed=MIX_SEED, **MIX)
    return tr


def _u8_run(u8, shards, prefetch, per_shard=12, batch=4):
    """two shards of 12 (3 batches each), epoch 0 whole, then two steps of epoch 1: per load the pixels, the crop plan and the mix plan"""
    import augref
    from test_gpu_input_u8 import expect
    tr = _u8_trainer(u8, per_shard, batch, prefetch, n_epochs=3)
    out = []
    try:
        per = per_shard // batch
        for epoch, steps in ((0, 2 * per), (1, 2)):
            for step in range(steps):
                tr.load_new_batch()
                assert tr.L.mi_batch_last_status(tr.c_batch) == 0
                sid, b = divmod(step, per)
                x, lab, pl = expect(shards, sid, b * batch, batch, per_shard, augref.RANDOM, 1, AUG_SEED, epoch, DIN, DOUT)
                p = tr.last_mix()
                assert _same_plan(p, _plan(MIX_SEED, epoch, tr.t.contents.cur_dump_id - 1, DOUT)), (epoch, step, p)
                got = tr.activation("input")
                assert np.array_equal(tr.last_plan(), pl) and np.array_equal(tr.labels(), lab)
                assert _same(got, R.mix(x, p)), "epoch %d step %d (prefetch %d)" % (epoch, step, prefetch)
                out.append((got, tr.last_plan(), p))
                tr.forward(); tr.backward(); tr.update()
                assert tr.check_errors() == 0
            if epoch == 0:
                tr.L.mi_trainer_end_epoch(tr.t, 0.0, 0.0, float(2 * per_shard))
    finally:
        tr.close()
    return out


def test_u8_shards_prefetch_on_and_off(tmp_path):
    from test_gpu_input_u8 import write_u8_shards
    shards, u8, _ = write_u8_shards(str(tmp_path), 2, 12, DIN, DOUT, seed=5)
    blocking, prefetched = _u8_run(u8, shards, False), _u8_run(u8, shards, True)
    assert len(blocking) == len(prefetched) == 8
    for (xa, pa, ma), (xb, pb, mb) in zip(blocking, prefetched):
        assert _same(xa, xb) and np.array_equal(pa, pb) and _same_plan(ma, mb)
    assert {m["mode"] for _, _, m in blocking} == {1, 2}


def test_dump_and_resume(tmp_path):
    from test_gpu_input_u8 import write_u8_shards
    per_shard, batch = 12, 4
    shards, u8, _ = write_u8_shards(str(tmp_path / "data"), 1, per_shard, DIN, DOUT, seed=11)
    root = str(tmp_path / "dumps")
    a = _u8_trainer(u8, per_shard, batch, False, root, dump_dir="run")
    try:
        for b in range(2):
            a.load_new_batch()
            a.forward(); a.backward()
            if b == 0:
                a.update()
        a.L.dump_trainer(5, a.t, b"run")  # in the middle of the second step: the next load is batch 2 of shard 0
        a.update()
        a.load_new_batch()
        want, want_mix, want_lab = a.activation("input"), a.last_mix(), a.labels()
        assert want_mix["mode"] != 0
    finally:
        a.close()
    b = _u8_trainer(u8, per_shard, batch, False, root, dump_dir="run")  # the mix setting is not dumped: set again
    try:
        b.L.overwrite_trainer_hyperparams(b.t, 5, b"run")
        b.load_new_batch()
        assert b.L.mi_batch_last_status(b.c_batch) == 0
        assert _same_plan(b.last_mix(), want_mix) and np.array_equal(b.labels(), want_lab)
        assert _same(b.activation("input"), want)
    finally:
        b.close()


# ---------------------------------------------------------------- rules
def test_refusals(params):
    tr = _trainer(params, 8, device=False)
    try:
        with pytest.raises(RuntimeError, match="MI_LOSS_DEVICE"):
            tr.set_mix()
        with pytest.raises(RuntimeError):
            tr.last_mix()
        tr.set_mix(mixup=0.0, cutmix=0.0)  # off is always allowed
        tr.set_loss(smoothing=0.1, device=True)
        for kw, word in ((dict(mixup=1.5), "alpha"), (dict(cutmix=-1.0), "alpha"), (dict(prob=1.5), "prob"), (dict(switch=-0.1), "switch_prob")):
            with pytest.raises(RuntimeError, match=word):
                tr.set_mix(**kw)
        tr.set_mix()
        with pytest.raises(RuntimeError, match="mixing"):
            tr.set_loss(smoothing=0.0, device=False)
        tr.set_loss(smoothing=0.0, device=True, copy_pred=False)  # the device head may change its settings
        assert tr.last_mix()["mode"] == 0  # nothing loaded yet
        tr.set_mix(mixup=0.0, cutmix=0.0)
        tr.set_loss(smoothing=0.0, device=False)
        tr.check()
    finally:
        tr.close()


def _names(L):
    buf = C.create_string_buffer(1 << 16)
    n = L.mi_debug_trace_names(buf, len(buf))
    names = buf.value.decode().split("\n")[:-1] if n else []
    assert n == len(names) < 96, "the launch ring is full (%d): launches were lost" % n
    return names


@pytest.mark.parametrize("mixing", [False, True])
def test_launches(params, mixing):
    """load_new_batch, forward_pass, backwards_pass and update_parameters looked at one by one (each fits the ring): with mixing never
    enabled no launch of a step names a mix kernel or the two-label head; with it on they are the load's last and the forward's head"""
    tr = _trainer(params, 8)
    try:
        if mixing:
            tr.set_mix(seed=_seed_with_both_modes(range(-1, 2), DIMS["input"]), **MIX)
        tr.source_synthetic()
        phases = []
        for call in (tr.load_new_batch, tr.forward, tr.backward, tr.update):
            tr.L.mi_debug_trace_clear()
            call()
            phases.append(_names(tr.L))
        assert tr.check_errors() == 0
        mode = tr.last_mix()["mode"] if mixing else 0
    finally:
        tr.close()
    mix_names = [n for ph in phases for n in ph if "mix" in n]
    if not mixing:
        assert mix_names == [] and "loss_head_kernel<reg>" in phases[1]
    else:
        kernel = {1: "mixup_kernel<vec>", 2: "cutmix_kernel<vec>"}[mode]
        assert phases[0][-2:] == [kernel, "mix_labels_kernel"]
        assert phases[1][-2:] == ["loss_head_mix_kernel<reg>", "loss_reduce_kernel"] and "loss_head_kernel<reg>" not in phases[1]
        assert mix_names == [kernel, "mix_labels_kernel", "loss_head_mix_kernel<reg>"]
