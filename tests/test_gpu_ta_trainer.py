"""TrivialAugmentWide in the trainer (mi_trainer_set_trivial_augment / mi_trainer_last_trivial_augment, include/resnet_mi.h
"TrivialAugmentWide") on C1S at batch 5 and 8 from the host source, on the synthetic source and on uint8 shards.

  images          after load_new_batch = tests/taref.py applied to an untouched twin's images under last_trivial_augment(), bit for bit,
                  and those records = the plan of the trainer's epoch / step; with erasing and mixing on: mix(erase(ta(x)))
  off             the batch bits and the launch ring are what they are without the call; on: the stage and the apply launch per load, in
                  front of the erase launch
  uint8 shards    prefetch on and off: the same pixels and records over four loads
  evaluation      eval_forward / evaluate_u8 records are equal with it on and off
  two full steps with LARS and smoothing; the refusals
"""
import ctypes as C

import numpy as np
import pytest

import eraseref
import mixref
import synth
import taref as R

pytestmark = pytest.mark.gpu

DIMS = synth.C1S_DIMS
DIN_NET = DIMS["input"]
L_OUT = DIMS["output"]
SCALE, RATIO = (0.02, 0.33), (0.3, 3.3)
ERASE = dict(mode="noise", value=(1.0, -2.0, 0.5), std=(58.395, 57.12, 57.375))
MIX = dict(mixup=0.8, cutmix=1.0, prob=1.0, switch=0.5)
PATH = "vec" if (DIN_NET * DIN_NET) % 4 == 0 else "elem"
TA_LAUNCHES = ["ta_stage_kernel<%s>" % PATH, "ta_apply_kernel<%s>" % PATH]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _key(rows):
    return [(r["op"], r["bin"], r["neg"], r["arg"], list(r["A"]), np.float32(r["factor"]).tobytes(), np.float64(r["magnitude"]).tobytes()) for r in rows]


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
    """NCHW images, fractions: the transform rounds them to bytes; -0.0 and a subnormal in every row"""
    x = synth.uniform(91, batch * 3 * DIN_NET * DIN_NET, -124.0, 152.0, offset=step * 100003).reshape(batch, 3, DIN_NET, DIN_NET).copy()
    x[:, 0, 0, :2] = [-0.0, 1e-45]
    return x, (np.arange(batch, dtype=np.int32) * 7 + step) % L_OUT


@pytest.mark.parametrize("batch", [5, 8])
def test_images_and_records_after_load(params, batch):
    from resnet_amd import binding as B
    seed = 17
    tr, twin = _trainer(params, batch), _trainer(params, batch)
    try:
        tr.set_trivial_augment(seed=seed)
        assert tr.last_trivial_augment() == []  # nothing loaded yet
        for t in (tr, twin):
            t.source_host(B.MI_LAYOUT_NCHW)
        ops_seen = set()
        for step in range(4):
            x, lab = _host_batch(batch, step)
            for t in (tr, twin):
                t.fill_host_batch(x, lab)
                t.load_new_batch()
            rows = tr.last_trivial_augment()
            # cur_dump_id before its increment: -1 at the first load
            assert _key(rows) == _key(R.plan(seed, 0, (step - 1) % 2 ** 64, 0, 1, batch, DIN_NET)), step
            plain, got = twin.activation("input"), tr.activation("input")
            assert _same(plain, x)
            assert _same(got, R.apply_batch(plain, rows)), "step %d" % step
            assert not _same(got, plain) and np.array_equal(tr.labels(), lab)
            ops_seen |= {r["op"] for r in rows}
            tr.forward(); tr.backward(); tr.update()
            assert tr.check_errors() == 0
        assert len(ops_seen) >= 8
        tr.check()
    finally:
        tr.close()
        twin.close()


def test_augment_then_erase_then_mix(params):
    batch, seed, eseed, mseed = 8, 3, 4, 5
    tr, twin = _trainer(params, batch, device=True, smoothing=0.1), _trainer(params, batch, device=True, smoothing=0.1)
    try:
        tr.set_mix(seed=mseed, **MIX)
        tr.set_erase(prob=1.0, seed=eseed, **ERASE)
        tr.set_trivial_augment(seed=seed)
        for t in (tr, twin):
            t.source_synthetic(pool_batches=3)
        fill = {k: v for k, v in ERASE.items() if k != "mode"}
        modes = set()
        for step in range(3):
            tr.load_new_batch()
            twin.load_new_batch()
            rows, boxes, p = tr.last_trivial_augment(), tr.last_erase(), tr.last_mix()
            assert _key(rows) == _key(R.plan(seed, 0, (step - 1) % 2 ** 64, 0, 1, batch, DIN_NET))
            assert np.array_equal(boxes, eraseref.plan(eseed, 0, step - 1, 0, 1, batch, DIN_NET, 1.0, SCALE, RATIO))
            plain = twin.activation("input")
            erase = lambda v: eraseref.erase(v, boxes, "noise", noise_seed=eraseref.step_key(eseed, 0, step - 1, 0, 1), **fill)
            want = mixref.mix(erase(R.apply_batch(plain, rows)), p)
            assert _same(tr.activation("input"), want), "step %d, mix mode %d" % (step, p["mode"])
            assert not _same(want, mixref.mix(R.apply_batch(erase(plain), rows), p))  # the order shows: the noise would be rounded to bytes
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


def test_launches_and_bits_with_it_off_and_on(params):
    """never called, and switched on and off again: the same launches and the same batch.  On: the two launches per load, behind the load
    and in front of the erase and mix launches"""
    def base(tr):
        tr.set_mix(seed=5, **MIX)
        tr.set_erase(prob=1.0, seed=1, **ERASE)
    never, x_never = _phases(params, base)

    def on_then_off(tr):
        base(tr)
        tr.set_trivial_augment(seed=1)
        tr.set_trivial_augment(on=False)
    off, x_off = _phases(params, on_then_off)
    assert off == never and _same(x_off, x_never)
    assert not [n for ph in never for n in ph if n.startswith("ta_")]

    def on(tr):
        base(tr)
        tr.set_trivial_augment(seed=1)
    with_ta, x_on = _phases(params, on)
    assert not _same(x_on, x_never)
    for load in (0, 4):
        at = never[load].index("erase_kernel<noise,vec>")
        assert with_ta[load] == never[load][:at] + TA_LAUNCHES + never[load][at:]
    assert with_ta[1:4] == never[1:4]
    alone, _ = _phases(params, lambda tr: tr.set_trivial_augment(seed=1))
    assert [n for n in alone[0] if n.startswith("ta_")] == TA_LAUNCHES and alone[0][-2:] == TA_LAUNCHES


# ---------------------------------------------------------------- uint8 shards
DIN, DOUT, AUG_SEED, TA_SEED = 40, 32, 4242, 9


def _u8_run(u8, shards, prefetch, per_shard=8, batch=4):
    """two shards of 8 (2 batches each): four loads over a shard boundary; per load the pixels, the crop plan and the records.  The source
    is bytes: quantise recovers them, and the result is the decode of Pillow's bytes on the crop"""
    import augref
    from test_gpu_input_u8 import expect, make_trainer
    tr = make_trainer(batch, per_shard)
    tr.source_shards_u8(u8, DIN, augment="random", flip=True, seed=AUG_SEED, prefetch=prefetch)
    tr.set_trivial_augment(seed=TA_SEED)
    out = []
    try:
        per = per_shard // batch
        for step in range(2 * per):
            tr.load_new_batch()
            assert tr.L.mi_batch_last_status(tr.c_batch) == 0
            sid, b = divmod(step, per)
            x, lab, pl = expect(shards, sid, b * batch, batch, per_shard, augref.RANDOM, 1, AUG_SEED, 0, DIN, DOUT)
            rows = tr.last_trivial_augment()
            assert _key(rows) == _key(R.plan(TA_SEED, 0, (tr.t.contents.cur_dump_id - 1) % 2 ** 64, 0, 1, batch, DOUT)), step
            got = tr.activation("input")
            assert np.array_equal(tr.last_plan(), pl) and np.array_equal(tr.labels(), lab)
            assert _same(R.decode(R.quantise(x)), x)  # a byte-valued source
            assert _same(got, R.apply_batch(x, rows)), "step %d (prefetch %d)" % (step, prefetch)
            out.append((got, _key(rows)))
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
    for (xa, ra), (xb, rb) in zip(blocking, prefetched):
        assert _same(xa, xb) and ra == rb


# ---------------------------------------------------------------- evaluation, full steps, rules
def test_eval_entry_points_never_augment(params):
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
                tr.set_trivial_augment(seed=4)
            tr.eval_metrics(reset=True)
            tr.eval_forward(ex, elab)
            fwd = tr.eval_metrics()[0]
            records.append((fwd, tr.evaluate_u8(images, labels, dim_in, topk=5)))
            assert _same(tr.activation("input"), x)
        tr.check()
        assert records[0] == records[1] and records[0][1]["rows"] == 2 * batch + 1 and np.isfinite(records[0][0]["loss_sum"])
    finally:
        tr.close()


def test_two_full_steps_with_lars_and_smoothing(params):
    tr = _trainer(params, 8, device=True, smoothing=0.1)
    try:
        tr.set_optimizer("lars")
        tr.set_trivial_augment(seed=2)
        tr.source_synthetic()
        for _ in range(2):
            tr.load_new_batch()
            tr.forward()
            last, _ = tr.metrics()
            assert np.isfinite(last["loss_sum"]) and last["loss_sum"] > 0 and last["rows"] == 8
            tr.backward()
            tr.update()
            assert tr.check_errors() == 0
            assert len(tr.last_trivial_augment()) == 8
        assert tr.error() == ""
        assert all(np.all(np.isfinite(tr.get("params", i))) for i in range(tr.n_locations))
    finally:
        tr.close()


def test_refusals(params):
    tr = _trainer(params, 8)
    try:
        with pytest.raises(RuntimeError, match="off"):
            tr.last_trivial_augment()
        tr.set_trivial_augment(on=False)  # off is always allowed
        with pytest.raises(RuntimeError, match="off"):
            tr.last_trivial_augment()
        tr.set_trivial_augment(seed=3)
        assert tr.last_trivial_augment() == []
        assert tr.L.mi_trainer_last_trivial_augment(tr.t, None) == -1
        tr.L.mi_clear_error()
        tr.set_trivial_augment(on=False)
        with pytest.raises(RuntimeError):
            tr.last_trivial_augment()
        tr.check()
    finally:
        tr.close()
