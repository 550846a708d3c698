"""The uint8 input path on the device (include/resnet_mi.h, "uint8 shards"): the decode kernel (kernels_input.hip) against the
reference binary's fixture and the numpy model (tests/augref.py), and load_new_batch from MI_SRC_SHARDS_U8 -- blocking and prefetched,
rank slices, epochs, resume -- against the same model.  Everything is compared bit for bit: the path moves bytes and looks floats up
in a table, nothing is summed."""
import hashlib
import os

import numpy as np
import pytest

import augref
import synth
from test_shards import DIM_IN, DIM_OUT, GOLD, N_CLASSES, ROWS, class_bytes

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7777.25)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- the kernel on its own
def test_decode_reproduces_the_reference_fixture(ops):
    """the FIXED plan of test_shards.ROWS at 256 -> 224 = the shard the REFERENCE binary wrote (tests/golden/shard_ref_golden.npz)"""
    classes = [class_bytes(c) for c in range(N_CLASSES)]
    src = np.stack([classes[c][n] for c, n, _, _ in ROWS])
    pl = augref.plan(augref.FIXED, 0, 0, 0, 0, len(ROWS), DIM_IN, DIM_OUT, [(r, s) for _, _, r, s in ROWS])
    out = ops.decode_u8(src, pl, DIM_OUT)
    assert np.array_equal(bits(out), bits(augref.decode(src, pl, DIM_OUT)))
    gold = np.load(os.path.join(GOLD, "shard_ref_golden.npz"))
    flat = out.ravel()
    assert flat.size == int(gold["n_floats"])
    assert np.array_equal(bits(flat[:64]), bits(gold["head"])) and np.array_equal(bits(flat[-64:]), bits(gold["tail"]))
    assert hashlib.sha256(flat.tobytes()).hexdigest() == str(gold["sha256"])


def sweep_plan(n, R, rng):
    """every col_off residue mod 4 (where R allows), both corners, flips mixed within the batch"""
    pl = np.zeros((n, 3), np.int32)
    for i in range(n):
        pl[i] = (rng.randint(0, R + 1), min(i % 4 + 4 * rng.randint(0, R // 4 + 1), R) if R >= 3 else rng.randint(0, R + 1), i % 2)
    pl[0] = (0, 0, 0)
    pl[-1] = (R, R, 1)
    if n > 4:
        pl[1] = (0, 0, 1)
        pl[2] = (R, R, 0)
    return pl


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("dim_in,dim_out", [(256, 224), (257, 224), (37, 30), (40, 33), (32, 32)])
def test_decode_sweep(ops, dim_in, dim_out, n):
    """odd dim_in (every source row starts at another byte residue), dim_out % 4 != 0 (scalar stores and tail), no crop at all;
    the output buffer is longer than the batch and pre-filled: nothing behind the last element may change"""
    rng = np.random.RandomState(dim_in * 1000 + dim_out + n)
    src = rng.randint(0, 256, size=(n, dim_in, dim_in, 3), dtype=np.uint8)
    pl = sweep_plan(n, dim_in - dim_out, rng)
    if dim_in - dim_out >= 3 and n >= 4:
        assert set(pl[:, 1] % 4) == {0, 1, 2, 3}
    out, pad = ops.decode_u8(src, pl, dim_out, pad_floats=1024, fill=SENTINEL)
    ref = augref.decode(src, pl, dim_out)
    bad = np.argwhere(bits(out) != bits(ref))
    assert bad.size == 0, "first mismatch at (n, d, h, w) = %s of %d" % (bad[0], len(bad))
    assert np.all(pad == SENTINEL)


def test_decode_refuses_an_unaligned_source(ops):
    src = ops.dev(np.zeros(64 * 64 * 3 + 16, np.uint8))
    pl = ops.dev(np.zeros((1, 3), np.int32))
    out = ops.dev(shape=(1, 3, 32, 32))
    assert ops.L.mi_op_decode_u8(src.ptr + 4, pl.ptr, out.ptr, 1, 64, 32) == -1
    assert "16-byte" in ops.L.mi_last_error().decode()
    ops.L.mi_clear_error()
    assert ops.L.mi_op_decode_u8(src.ptr, pl.ptr, out.ptr, 1, 64, 32) == 0


# ---------------------------------------------------------------- the loader
def write_u8_shards(root, n_shards, per_shard, dim_in, dim_out, seed=0):
    """class files + partition CSVs -> mi_build_shard_u8 (and mi_build_shard, for the drop-in check) -> per shard (images, labels, crops)"""
    from resnet_amd import binding as B
    lib = B.load()
    rng = np.random.RandomState(seed)
    n_classes, per_class = 3, 6
    data, part, u8, f32 = (os.path.join(root, d) for d in ("classes", "part", "u8", "f32"))
    for d in (data, part, u8, f32):
        os.makedirs(d)
    classes = rng.randint(0, 256, size=(n_classes, per_class, dim_in, dim_in, 3), dtype=np.uint8)
    for c in range(n_classes):
        classes[c].tofile(os.path.join(data, "%08d.buffer" % c))
    shards = []
    for sid in range(n_shards):
        rows = [(rng.randint(n_classes), rng.randint(per_class), rng.randint(dim_in - dim_out + 1), rng.randint(dim_in - dim_out + 1))
                for _ in range(per_shard)]
        csv = os.path.join(part, "%03d_images.csv" % sid)
        with open(csv, "w") as f:
            for r in rows:
                f.write("%03d,%04d,%02d,%02d\n" % r)
        assert lib.mi_build_shard_u8(csv.encode(), data.encode(), u8.encode(), sid, dim_in) == per_shard
        assert lib.mi_build_shard(csv.encode(), data.encode(), f32.encode(), sid, dim_in, dim_out, B.MI_LAYOUT_NCHW) == per_shard
        shards.append((np.stack([classes[c][k] for c, k, _, _ in rows]), np.array([r[0] for r in rows], np.int32),
                       np.array([r[2:] for r in rows], np.int32)))
    return shards, u8, f32


def make_trainer(batch, per_shard, dims=synth.C1_DIMS, **kw):
    from resnet_amd import Trainer
    tr = Trainer(dims, batch, seed=1236, shard_n_images=per_shard, **kw)
    if tr.L.mi_device_count() < 1:
        pytest.fail("needs the MI355X box")
    return tr


def expect(shards, sid, first_in_shard, n, per_shard, mode, flip, seed, epoch, dim_in, dim_out):
    """(input, labels, plan) of images [first_in_shard, + n) of shard sid"""
    img, lab, crops = shards[sid]
    sl = slice(first_in_shard, first_in_shard + n)
    pl = augref.plan(mode, flip, seed, epoch, sid * per_shard + first_in_shard, n, dim_in, dim_out, crops[sl])
    return augref.decode(img[sl], pl, dim_out), lab[sl], pl


DIN, DOUT, SEED = 40, 32, 4242


def run_loader(u8_dir, shards, prefetch, steps, per_shard=24, batch=4):
    tr = make_trainer(batch, per_shard)
    losses = []
    try:
        tr.L.mi_trainer_set_input_reset(tr.t, 1)
        tr.source_shards_u8(u8_dir, DIN, augment="random", flip=True, seed=SEED, prefetch=prefetch)
        per = per_shard // batch
        inputs = []
        for step in range(steps):
            tr.load_new_batch()
            assert tr.L.mi_batch_last_status(tr.c_batch) == 0
            sid, b = divmod(step, per)
            x, lab, pl = expect(shards, sid, b * batch, batch, per_shard, augref.RANDOM, 1, SEED, 0, DIN, DOUT)
            got = tr.activation("input")
            assert np.array_equal(tr.last_plan(), pl), "step %d" % step
            assert np.array_equal(bits(got), bits(x)), "step %d" % step
            assert np.array_equal(tr.labels(), lab)
            assert tr.c_batch.contents.cur_shard_id == sid and tr.t.contents.cur_dump_id == step
            inputs.append(got)
            tr.forward()
            losses.append(tr.loss()[0])
            tr.backward()
            tr.update()
        tr.check()
        tr.load_new_batch()  # the third shard does not exist
        assert tr.L.mi_batch_last_status(tr.c_batch) == -1
    finally:
        tr.close()
    return inputs, losses


def test_loader_random_crops_blocking_and_prefetched(tmp_path):
    """two shards of 24 images, 40 -> 32, batch 4, RANDOM with flips; full training steps with input_reset on between the loads"""
    shards, u8, _ = write_u8_shards(str(tmp_path), 2, 24, DIN, DOUT)
    xa, la = run_loader(u8, shards, False, 12)
    xb, lb = run_loader(u8, shards, True, 12)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(xa, xb))
    assert la == lb and all(np.isfinite(la))
    assert any(p[2] for x in range(6) for p in augref.plan(augref.RANDOM, 1, SEED, 0, 4 * x, 4, DIN, DOUT))  # flips do occur


def test_fixed_mode_is_a_drop_in_for_the_fp32_shards(tmp_path):
    """FIXED crops from the uint8 shard = the fp32 shard mi_build_shard writes from the same CSV: same inputs, same training"""
    from resnet_amd import binding as B
    per_shard, batch = 8, 4
    shards, u8, f32 = write_u8_shards(str(tmp_path), 1, per_shard, DIN, DOUT, seed=3)
    runs = []
    for kind in ("u8", "f32"):
        tr = make_trainer(batch, per_shard)
        try:
            if kind == "u8":
                tr.source_shards_u8(u8, DIN, augment="fixed")
            else:
                tr.source_shards(f32, B.MI_LAYOUT_NCHW)
            rec = []
            for step in range(2):
                tr.load_new_batch()
                assert tr.L.mi_batch_last_status(tr.c_batch) == 0
                x = tr.activation("input")
                tr.forward()
                loss = tr.loss()[0]
                tr.backward()
                grads = [tr.get("grads", i) for i in range(tr.n_locations)]
                tr.update()
                rec.append((x, tr.labels(), loss, grads))
            tr.check()
            runs.append(rec)
        finally:
            tr.close()
    for (xa, la, lossa, ga), (xb, lb, lossb, gb) in zip(*runs):
        assert np.array_equal(bits(xa), bits(xb)) and np.array_equal(la, lb)
        assert lossa == lossb and np.isfinite(lossa)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(ga, gb))
    x0, _, pl0 = expect(shards, 0, 0, batch, per_shard, augref.FIXED, 0, 0, 0, DIN, DOUT)
    assert np.array_equal(bits(runs[0][0][0]), bits(x0))


def test_fixed_mode_needs_the_crops_file(tmp_path):
    shards, u8, _ = write_u8_shards(str(tmp_path), 1, 8, DIN, DOUT)
    os.remove(os.path.join(u8, "000.crops"))
    tr = make_trainer(4, 8)
    try:
        tr.source_shards_u8(u8, DIN, augment="fixed")
        tr.load_new_batch()
        assert tr.L.mi_batch_last_status(tr.c_batch) == -1
    finally:
        tr.close()
    tr = make_trainer(4, 8)
    try:
        tr.source_shards_u8(u8, DIN, augment="center")  # no crops needed
        tr.load_new_batch()
        assert tr.L.mi_batch_last_status(tr.c_batch) == 0
        x, _, pl = expect(shards, 0, 0, 4, 8, augref.CENTER, 0, 0, 0, DIN, DOUT)
        assert np.array_equal(tr.last_plan(), pl) and np.array_equal(bits(tr.activation("input")), bits(x))
    finally:
        tr.close()


def test_set_augment_is_for_u8_shards_only():
    from resnet_amd import binding as B
    tr = make_trainer(4, 8)
    try:
        tr.source_synthetic()
        assert tr.L.mi_batch_set_augment(tr.c_batch, B.MI_AUG_RANDOM, 1, 5) == -1
        assert "MI_SRC_SHARDS_U8" in tr.error()
        tr.L.mi_clear_error()
        with pytest.raises(RuntimeError):
            tr.last_plan()
    finally:
        tr.close()


@pytest.mark.parametrize("prefetch", [False, True])
def test_rank_slices(tmp_path, prefetch):
    """world 2: rank r decodes the images of its slice of every global batch, drawn at their GLOBAL indices; both ranks roll to the
    next shard at the same step (a ragged tail of 4 of 20 images is skipped)"""
    N, W, per_shard = 4, 2, 20
    shards, u8, _ = write_u8_shards(str(tmp_path), 2, per_shard, DIN, DOUT, seed=9)
    trs = []
    try:
        for r in range(W):
            tr = make_trainer(N, per_shard)
            tr.source_shards_u8(u8, DIN, augment="random", flip=True, seed=SEED, prefetch=prefetch)
            tr.L.mi_batch_set_rank_slice(tr.c_batch, r, W)
            trs.append(tr)
        per = per_shard // (W * N)
        for step in range(2 * per):
            sid, g = divmod(step, per)
            for r, tr in enumerate(trs):
                tr.load_new_batch()
                assert tr.L.mi_batch_last_status(tr.c_batch) == 0
                x, lab, pl = expect(shards, sid, (g * W + r) * N, N, per_shard, augref.RANDOM, 1, SEED, 0, DIN, DOUT)
                assert np.array_equal(tr.last_plan(), pl), (step, r)
                assert np.array_equal(bits(tr.activation("input")), bits(x)), (step, r)
                assert np.array_equal(tr.labels(), lab)
                assert tr.c_batch.contents.cur_shard_id == sid
                if prefetch:
                    tr.forward(); tr.backward(); tr.update()
    finally:
        for tr in trs:
            tr.close()


@pytest.mark.parametrize("prefetch", [False, True])
def test_epochs_draw_anew_and_a_resumed_run_sees_the_same_pixels(tmp_path, prefetch):
    per_shard, batch = 12, 4
    shards, u8, _ = write_u8_shards(str(tmp_path / "data"), 1, per_shard, DIN, DOUT, seed=11)
    root = str(tmp_path / "dumps")

    def fresh():
        tr = make_trainer(batch, per_shard, dump_dir="run", n_epochs=3)
        tr.L.mi_trainer_set_dump_root(tr.t, root.encode())
        tr.source_shards_u8(u8, DIN, augment="random", flip=True, seed=SEED, prefetch=prefetch)
        return tr

    a = fresh()
    try:
        epoch0 = []
        for b in range(3):  # epoch 0: the whole shard
            a.load_new_batch()
            epoch0.append(a.activation("input"))
            a.forward(); a.backward(); a.update()
        a.L.mi_trainer_end_epoch(a.t, 0.0, 0.0, float(per_shard))
        assert a.t.contents.cur_epoch == 1
        for b in range(2):  # epoch 1: shard 0 again, other pixels
            a.load_new_batch()
            assert a.L.mi_batch_last_status(a.c_batch) == 0
            x, lab, pl = expect(shards, 0, b * batch, batch, per_shard, augref.RANDOM, 1, SEED, 1, DIN, DOUT)
            got = a.activation("input")
            assert np.array_equal(a.last_plan(), pl) and np.array_equal(bits(got), bits(x)), b
            assert not np.array_equal(bits(got), bits(epoch0[b]))
            a.forward(); a.backward()
            if b == 0:
                a.update()
        a.L.dump_trainer(5, a.t, b"run")  # in the middle of step 2 of epoch 1: the next load is batch 2 of shard 0
        a.update()
        a.load_new_batch()
        want, want_plan, want_lab = a.activation("input"), a.last_plan(), a.labels()
        x, lab, pl = expect(shards, 0, 2 * batch, batch, per_shard, augref.RANDOM, 1, SEED, 1, DIN, DOUT)
        assert np.array_equal(bits(want), bits(x)) and np.array_equal(want_plan, pl)
    finally:
        a.close()

    b = fresh()  # seed and mode are not dumped: fresh() sets them again
    try:
        b.L.overwrite_trainer_hyperparams(b.t, 5, b"run")
        assert b.t.contents.init_loaded == 1 and b.t.contents.cur_epoch == 1 and b.c_batch.contents.cur_batch_in_shard == 2
        b.load_new_batch()
        assert b.L.mi_batch_last_status(b.c_batch) == 0
        assert np.array_equal(b.last_plan(), want_plan) and np.array_equal(b.labels(), want_lab)
        assert np.array_equal(bits(b.activation("input")), bits(want))
    finally:
        b.close()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_full_size_step(tmp_path, dtype):
    """ResNet-50 at 224^2, batch 8, from a 256^2 uint8 shard: one full step, the stems read what the decode wrote"""
    from resnet_amd import binding as B
    per_shard, batch = 16, 8
    shards, u8, _ = write_u8_shards(str(tmp_path), 1, per_shard, 256, 224, seed=21)
    tr = make_trainer(batch, per_shard, dims=synth.R50_DIMS)
    try:
        if dtype == "bf16":
            tr.set_dtype(B.MI_DTYPE_BF16)
        tr.source_shards_u8(u8, 256, augment="random", flip=True, seed=SEED, prefetch=True)
        for step in range(2):
            tr.load_new_batch()
            assert tr.L.mi_batch_last_status(tr.c_batch) == 0
            x, lab, pl = expect(shards, 0, step * batch, batch, per_shard, augref.RANDOM, 1, SEED, 0, 256, 224)
            assert np.array_equal(tr.last_plan(), pl) and np.array_equal(tr.labels(), lab)
            assert np.array_equal(bits(tr.activation("input")), bits(x)), step
            tr.forward()
            loss = tr.loss()[0]
            tr.backward()
            tr.update()
            assert tr.check_errors() == 0
            tr.check()
            assert np.isfinite(loss)
    finally:
        tr.close()
