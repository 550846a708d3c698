"""Random erasing in the trainer (mi_trainer_set_erase / mi_trainer_last_erase, include/resnet_mi.h "random erasing") on C1S at batch 5
and 8 from the host source, on the synthetic source and on uint8 shards.

  images          after load_new_batch = the numpy erase (tests/eraseref.py) of an untouched twin's images under last_erase(), bit for bit,
                  and last_erase() = the plan of the trainer's epoch / step; with mixing on: mixref.mix(eraseref.erase(x))
  off             the batch bits and the launch ring are what they are without the call; on: one erase launch per load, in front of the mix
  uint8 shards    prefetch on and off: the same pixels and boxes over four loads; dump and resume
  evaluation      eval_forward / evaluate_u8 records are equal with erasing on and off
  two full steps with LARS, smoothing and erasing; the refusals
"""
import ctypes as C

import numpy as np
import pytest

import eraseref as R
import mixref
import synth

pytestmark = pytest.mark.gpu

DIMS = synth.C1S_DIMS
DIN_NET = DIMS["input"]
L_OUT = DIMS["output"]
SCALE, RATIO = (0.02, 0.33), (0.3, 3.3)
FILLS = {"const": dict(mode="const", value=(-0.0, 3.5, -7.25)), "noise": dict(mode="noise", value=(1.0, -2.0, 0.5), std=(58.395, 57.12, 57.375))}
MIX = dict(mixup=0.8, cutmix=1.0, prob=1.0, switch=0.5)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def params():
    return synth.make_params(DIMS, perturb_bn=True)


def _trainer(params, batch, device=False, smoothing=0.0):
    from resnet_amd import Trainer
    tr = Trainer(DIMS, batch)
    if tr.L.mi_device_count() < 1:
        pytest.fail("no HIP device: this test must run on the MI355X box")
    tr.set_params(params)
    if device:
        tr.set_loss(smoothing=smoothing, topk=5, device=True)
    return tr


def _host_batch(batch, step=0):
    """NCHW images with -0.0 and a subnormal in every row (all finite: the batches are trained on)"""
    x = synth.uniform(91, batch * 3 * DIN_NET * DIN_NET, -124.0, 152.0, offset=step * 100003).reshape(batch, 3, DIN_NET, DIN_NET).copy()
    x[:, 0, 0, :2] = [-0.0, 1e-45]
    return x, (np.arange(batch, dtype=np.int32) * 7 + step) % L_OUT


def _erased(x, boxes, fill, seed, epoch, step, rank=0, world=1):
    """what the trainer's erase step makes of x: noise_seed = the plan's e, first_row = 0"""
    f = {k: v for k, v in FILLS[fill].items() if k != "mode"}
    return R.erase(x, boxes, fill, noise_seed=R.step_key(seed, epoch, step, rank, world), **f)


@pytest.mark.parametrize("fill", ["const", "noise"])
@pytest.mark.parametrize("batch", [5, 8])
def test_images_and_boxes_after_load(params, batch, fill):
    from resnet_amd import binding as B
    seed = 17
    tr, twin = _trainer(params, batch), _trainer(params, batch)
    try:
        tr.set_erase(prob=1.0, seed=seed, **FILLS[fill])
        assert tr.last_erase().shape == (0, 4)  # nothing loaded yet
        for t in (tr, twin):
            t.source_host(B.MI_LAYOUT_NCHW)
        for step in range(3):
            x, lab = _host_batch(batch, step)
            for t in (tr, twin):
                t.fill_host_batch(x, lab)
                t.load_new_batch()
            boxes = tr.last_erase()
            # cur_dump_id before its increment: -1 at the first load
            assert np.array_equal(boxes, R.plan(seed, 0, step - 1, 0, 1, batch, DIN_NET, 1.0, SCALE, RATIO)), step
            assert np.all((boxes[:, 2] > 0) & (boxes[:, 3] > 0))
            plain, got = twin.activation("input"), tr.activation("input")
            assert _same(plain, x)
            assert _same(got, _erased(plain, boxes, fill, seed, 0, step - 1)), "step %d" % step
            assert not _same(got, plain) and np.array_equal(tr.labels(), lab)
            tr.forward(); tr.backward(); tr.update()  # the host head: no label changes, nothing else to set
            assert tr.check_errors() == 0
        tr.check()
    finally:
        tr.close()
        twin.close()


def test_erase_runs_in_front_of_the_mix(params):
    batch, seed, mseed = 8, 3, 5
    tr, twin = _trainer(params, batch, device=True, smoothing=0.1), _trainer(params, batch, device=True, smoothing=0.1)
    try:
        tr.set_mix(seed=mseed, **MIX)
        tr.set_erase(prob=1.0, seed=seed, **FILLS["noise"])
        for t in (tr, twin):
            t.source_synthetic(pool_batches=3)
        modes = set()
        for step in range(3):
            tr.load_new_batch()
            twin.load_new_batch()
            boxes, p = tr.last_erase(), tr.last_mix()
            assert np.array_equal(boxes, R.plan(seed, 0, step - 1, 0, 1, batch, DIN_NET, 1.0, SCALE, RATIO))
            plain = twin.activation("input")
            erased = _erased(plain, boxes, "noise", seed, 0, step - 1)
            want = mixref.mix(erased, p)
            assert _same(tr.activation("input"), want), "step %d, mix mode %d" % (step, p["mode"])
            if p["mode"] != 0:
                assert not _same(want, _erased(mixref.mix(plain, p), boxes, "noise", seed, 0, step - 1))  # the order shows
            modes.add(p["mode"])
            tr.forward(); tr.backward(); tr.update()
            assert tr.check_errors() == 0
        assert modes - {0}
        tr.check()
    finally:
        tr.close()
        twin.close()


def _names(L):
    buf = C.create_string_buffer(1 << 16)
    n = L.mi_debug_trace_names(buf, len(buf))
    names = buf.value.decode().split("\n")[:-1] if n else []
    assert n == len(names) < 96, "the launch ring is full (%d): launches were lost" % n
    return names


def _phases(params, setup):
    tr = _trainer(params, 8, device=True)
    try:
        setup(tr)
        tr.source_synthetic()
        phases = []
        for call in (tr.load_new_batch, tr.forward, tr.backward, tr.update, tr.load_new_batch):
            tr.L.mi_debug_trace_clear()
            call()
            phases.append(_names(tr.L))
        assert tr.check_errors() == 0
        tr.check()
        return phases, tr.activation("input")
    finally:
        tr.close()


def test_launches_and_bits_with_erasing_off_and_on(params):
    """never called, and switched on and off again: the same launches and the same batch.  On: one erase launch per load, behind the
    load and in front of the mix launches"""
    never, x_never = _phases(params, lambda tr: tr.set_mix(seed=5, **MIX))

    def on_then_off(tr):
        tr.set_mix(seed=5, **MIX)
        tr.set_erase(prob=0.5, seed=1, **FILLS["noise"])
        tr.set_erase(prob=0.0)
    off, x_off = _phases(params, on_then_off)
    assert off == never and _same(x_off, x_never)
    assert not [n for ph in never for n in ph if "erase" in n]

    def on(tr):
        tr.set_mix(seed=5, **MIX)
        tr.set_erase(prob=1.0, seed=1, **FILLS["noise"])
    with_erase, x_on = _phases(params, on)
    assert not _same(x_on, x_never)
    for load in (0, 4):
        mixed = [n for n in never[load] if "mix" in n]
        assert mixed and with_erase[load][-len(mixed):] == mixed
        assert with_erase[load][-len(mixed) - 1] == "erase_kernel<noise,vec>"
        assert with_erase[load] == never[load][:-len(mixed)] + ["erase_kernel<noise,vec>"] + mixed
    assert with_erase[1:4] == never[1:4]
    alone, _ = _phases(params, lambda tr: tr.set_erase(prob=1.0, seed=1, **FILLS["const"]))
    assert [n for n in alone[0] if "erase" in n] == ["erase_kernel<const,vec>"] and alone[0][-1] == "erase_kernel<const,vec>"


# ---------------------------------------------------------------- uint8 shards
DIN, DOUT, AUG_SEED, ERASE_SEED = 40, 32, 4242, 9


def _u8_trainer(u8, per_shard, batch, prefetch, root=None, **kw):
    from test_gpu_input_u8 import make_trainer
    tr = make_trainer(batch, per_shard, **kw)
    if root:
        tr.L.mi_trainer_set_dump_root(tr.t, root.encode())
    tr.source_shards_u8(u8, DIN, augment="random", flip=True, seed=AUG_SEED, prefetch=prefetch)
    tr.set_erase(prob=0.7, seed=ERASE_SEED, **FILLS["noise"])
    return tr


def _u8_run(u8, shards, prefetch, per_shard=8, batch=4):
    """two shards of 8 (2 batches each): four loads over a shard boundary; per load the pixels, the crop plan and the boxes"""
    import augref
    from test_gpu_input_u8 import expect
    tr = _u8_trainer(u8, per_shard, batch, prefetch)
    out = []
    try:
        per = per_shard // batch
        for step in range(2 * per):
            tr.load_new_batch()
            assert tr.L.mi_batch_last_status(tr.c_batch) == 0
            sid, b = divmod(step, per)
            x, lab, pl = expect(shards, sid, b * batch, batch, per_shard, augref.RANDOM, 1, AUG_SEED, 0, DIN, DOUT)
            boxes = tr.last_erase()
            assert np.array_equal(boxes, R.plan(ERASE_SEED, 0, tr.t.contents.cur_dump_id - 1, 0, 1, batch, DOUT, 0.7, SCALE, RATIO)), step
            got = tr.activation("input")
            assert np.array_equal(tr.last_plan(), pl) and np.array_equal(tr.labels(), lab)
            assert _same(got, _erased(x, boxes, "noise", ERASE_SEED, 0, tr.t.contents.cur_dump_id - 1)), "step %d (prefetch %d)" % (step, prefetch)
            out.append((got, boxes))
            tr.forward(); tr.backward(); tr.update()
            assert tr.check_errors() == 0
        tr.check()
    finally:
        tr.close()
    return out


def test_u8_shards_prefetch_on_and_off(tmp_path):
    from test_gpu_input_u8 import write_u8_shards
    shards, u8, _ = write_u8_shards(str(tmp_path), 2, 8, DIN, DOUT, seed=5)
    blocking, prefetched = _u8_run(u8, shards, False), _u8_run(u8, shards, True)
    assert len(blocking) == len(prefetched) == 4
    for (xa, ba), (xb, bb) in zip(blocking, prefetched):
        assert _same(xa, xb) and np.array_equal(ba, bb)
    erased = np.concatenate([b[:, 2] * b[:, 3] > 0 for _, b in blocking])
    assert erased.any() and not erased.all()  # prob 0.7 on 16 rows: both kinds of row were seen


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
        want, want_boxes = a.activation("input"), a.last_erase()
        assert np.any(want_boxes[:, 2] * want_boxes[:, 3] > 0)
    finally:
        a.close()
    b = _u8_trainer(u8, per_shard, batch, False, root, dump_dir="run")  # the erase setting is not dumped: set again
    try:
        b.L.overwrite_trainer_hyperparams(b.t, 5, b"run")
        b.load_new_batch()
        assert b.L.mi_batch_last_status(b.c_batch) == 0
        assert np.array_equal(b.last_erase(), want_boxes) and _same(b.activation("input"), want)
    finally:
        b.close()


# ---------------------------------------------------------------- evaluation, full steps, rules
def test_eval_entry_points_never_erase(params):
    from resnet_amd import binding as B
    batch, dim_in = 4, 40
    rng = np.random.RandomState(3)
    images = rng.randint(0, 256, size=(2 * batch + 1, dim_in, dim_in, 3)).astype(np.uint8)
    labels = rng.randint(0, L_OUT, size=2 * batch + 1).astype(np.int32)
    tr = _trainer(params, batch)
    try:
        tr.track_running_stats(1.0)
        tr.source_host(B.MI_LAYOUT_NCHW)
        x, lab = _host_batch(batch)
        tr.fill_host_batch(x, lab)
        tr.load_new_batch()
        tr.forward()
        tr.check()
        ex, elab = _host_batch(batch, 5)
        records = []
        for on in (False, True):
            if on:
                tr.set_erase(prob=1.0, seed=4, **FILLS["const"])
            tr.eval_metrics(reset=True)
            tr.eval_forward(ex, elab)
            fwd = tr.eval_metrics()[0]
            records.append((fwd, tr.evaluate_u8(images, labels, dim_in, topk=5)))
            assert _same(tr.activation("input"), x)
        tr.check()
        assert records[0] == records[1] and records[0][1]["rows"] == 2 * batch + 1 and np.isfinite(records[0][0]["loss_sum"])
    finally:
        tr.close()


@pytest.mark.parametrize("fill", ["const", "noise"])
def test_two_full_steps_with_lars_and_smoothing(params, fill):
    tr = _trainer(params, 8, device=True, smoothing=0.1)
    try:
        tr.set_optimizer("lars")
        tr.set_erase(prob=1.0, seed=2, **FILLS[fill])
        tr.source_synthetic()
        for _ in range(2):
            tr.load_new_batch()
            tr.forward()
            last, _ = tr.metrics()
            assert np.isfinite(last["loss_sum"]) and last["loss_sum"] > 0 and last["rows"] == 8
            tr.backward()
            tr.update()
            assert tr.check_errors() == 0
            assert tr.last_erase().shape == (8, 4)
        assert tr.error() == ""
        assert all(np.all(np.isfinite(tr.get("params", i))) for i in range(tr.n_locations))
    finally:
        tr.close()


def test_refusals(params):
    nan, inf = float("nan"), float("inf")
    tr = _trainer(params, 8)
    try:
        with pytest.raises(RuntimeError, match="off"):
            tr.last_erase()
        tr.set_erase(prob=0.0)  # off is always allowed
        for kw, word in ((dict(prob=1.5), "prob"), (dict(prob=-0.1), "prob"), (dict(prob=nan), "prob"), (dict(scale=(0.0, 0.3)), "scale_lo"),
                         (dict(scale=(0.4, 0.3)), "scale_hi"), (dict(ratio=(-1.0, 3.3)), "ratio_lo"), (dict(ratio=(3.0, 0.3)), "ratio_hi"),
                         (dict(mode=2), "mode"), (dict(value=(0, nan, 0)), "finite"), (dict(std=(inf, 1, 1)), "finite"), (dict(std=(1, 1, -1)), "negative")):
            with pytest.raises(RuntimeError, match=word):
                tr.set_erase(**kw)
            with pytest.raises(RuntimeError):
                tr.last_erase()  # a refused call leaves it off
        assert tr.L.mi_trainer_set_erase(tr.t, 0.5, 0.02, 0.33, 0.3, 3.3, None, 0) == -1
        assert "fill" in tr.error()
        tr.L.mi_clear_error()
        tr.set_erase()
        assert tr.last_erase().shape == (0, 4)
        with pytest.raises(RuntimeError, match="prob"):
            tr.set_erase(prob=2.0)
        assert tr.last_erase().shape == (0, 4)  # a refused change keeps the setting
        tr.set_erase(prob=0.0)
        with pytest.raises(RuntimeError):
            tr.last_erase()
        tr.check()
    finally:
        tr.close()
