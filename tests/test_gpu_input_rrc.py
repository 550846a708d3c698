"""The random-resized crop on the device (include/resnet_mi.h, "random-resized crop"): the resample kernel (kernels_input.hip) against
the numpy model (tests/rrcref.py) and against the decode kernel, and load_new_batch in MI_AUG_RRC mode -- blocking and prefetched, epochs,
rank slices, resume, switching back -- against the same model.  Everything is compared bit for bit: the arithmetic is integer up to one
exactly specified conversion."""
import os

import numpy as np
import pytest

import augref
import rrcref
import synth
from test_gpu_input_u8 import SENTINEL, bits, make_trainer, write_u8_shards

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the kernel on its own
def sweep_boxes(n, dim_in, D, rng):
    """the boxes the kernel can go wrong on, one batch; the LAST image's box is flush with the bottom-right corner, so its last span
    ends with the batch (the guarded 16-byte load)"""
    small = max(dim_in // 3, 1)
    if n == 1:
        return np.array([(dim_in - small, dim_in - 7, small, 7, 1)], np.int32)
    bx = [(0, 0, 1, 1, 0), (dim_in - 1, dim_in - 1, 1, 1, 1),                                  # 1 x 1
          (5, 0, 1, dim_in, 1), (0, 7, dim_in, 1, 0), (dim_in - 1, 2, 1, small, 0),            # 1 x w, h x 1
          (0, 0, dim_in, dim_in, 0), (0, 0, dim_in, dim_in, 1),                                # the whole image: the strongest downscale
          (0, 0, small, 11, 0), (0, dim_in - 11, small, 11, 1), (dim_in - small, 0, small, 11, 1),  # corners (the fourth closes the batch)
          (3, 4, 2, 3, 0), (dim_in - 4, 1, 3, 2, 1),                                           # strong upscaling
          (-5, dim_in + 3, 0, 900, 7), (1000, -1000, 2 * dim_in, 3, 1), (2, 2, -4, -4, 0),     # out of range: clamped
          (dim_in - min(D, dim_in), 0, D, D, 1), (0, dim_in - min(D, dim_in), D, D, 0)]        # exactly dim_out (clamped where dim_in < D)
    w16 = dim_in - 15
    for c0 in range(16):  # the span's first byte is 3 col0 + a constant: col0 = 0 .. 15 takes every residue mod 16
        h = rng.randint(1, dim_in + 1)
        bx.append((rng.randint(0, dim_in - h + 1), c0, h, rng.randint(1, w16 + 1), c0 & 1))
    assert len(bx) == n
    bx[4], bx[-1] = bx[-1], (dim_in - small, dim_in - 11, small, 11, 0)
    return np.array(bx, np.int32)


def run_resample(ops, src, boxes, D, front=1024, back=1024):
    """mi_op_resample_u8 into the middle of a pre-filled buffer -> (images, the floats in front, the floats behind)"""
    n, dim_in = src.shape[0], src.shape[1]
    total = n * 3 * D * D
    dsrc, dbox = ops.dev(src), ops.dev(np.ascontiguousarray(boxes, np.int32))
    dout = ops.dev(np.full(front + total + back, SENTINEL, np.float32))
    rc = ops.L.mi_op_resample_u8(dsrc.ptr, dbox.ptr, dout.ptr + 4 * front, n, dim_in, D)
    assert rc == 0, ops.L.mi_last_error().decode()
    out = dout.get()
    return out[front:front + total].reshape(n, 3, D, D), out[:front], out[front + total:]


def check(out, ref):
    bad = np.argwhere(bits(out) != bits(ref))
    assert bad.size == 0, "first mismatch at (n, d, h, w) = %s of %d" % (bad[0], len(bad))


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("dim_in,dim_out", [(256, 224), (257, 224), (37, 30), (40, 33), (32, 32)])
def test_resample_sweep(ops, dim_in, dim_out, n):
    """odd dim_in (every source row starts at another byte residue), dim_out % 4 != 0 (scalar stores and tail), dim_in == dim_out"""
    rng = np.random.RandomState(dim_in * 1000 + dim_out + n)
    src = rng.randint(0, 256, size=(n, dim_in, dim_in, 3), dtype=np.uint8)
    boxes = sweep_boxes(n, dim_in, dim_out, rng)
    cl = np.array([rrcref.clamp_box(b, dim_in) for b in boxes])
    assert np.array_equal(cl[-1, :2] + cl[-1, 2:4], (dim_in, dim_in))  # the last box ends with the batch
    if n > 1:
        assert set((3 * cl[:, 1]) % 16) == set(range(16)) and set(cl[:, 4]) == {0, 1}
        assert cl[:, 2:4].min() == 1 and cl[:, 2:4].max() == dim_in and any(np.array_equal(b[2:4], (min(dim_out, dim_in),) * 2) for b in cl)
        assert not np.array_equal(cl, boxes)  # some were out of range
    out, front, back = run_resample(ops, src, boxes, dim_out)
    check(out, rrcref.resample(src, boxes, dim_out))
    check(out, rrcref.resample(src, cl, dim_out))
    assert np.all(front == SENTINEL) and np.all(back == SENTINEL)


def test_resample_into_an_unaligned_output(ops):
    """dim_out % 4 == 0 but out 4 bytes off a 16-byte boundary: the scalar stores"""
    rng = np.random.RandomState(77)
    dim_in, D, n = 40, 32, 3
    src = rng.randint(0, 256, size=(n, dim_in, dim_in, 3), dtype=np.uint8)
    boxes = np.array([(0, 0, 40, 40, 1), (7, 9, 13, 21, 0), (8, 8, 32, 32, 1)], np.int32)
    out, front, back = run_resample(ops, src, boxes, D, front=1021, back=1027)
    check(out, rrcref.resample(src, boxes, D))
    assert np.all(front == SENTINEL) and np.all(back == SENTINEL)


WIDE_IN, WIDE_OUT = 344, 260


def wide_boxes():
    """the boxes of test_resample_wide_output_and_wide_box: 340 columns from column 0 and from column 3 (another residue of the span's
    first byte), flipped and not; the whole image; a narrow box for comparison"""
    return np.array([(2, 0, 340, 340, 0), (0, 3, 300, 340, 1), (0, 0, WIDE_IN, WIDE_IN, 1), (5, 7, 60, 50, 0)], np.int32)


def test_resample_wide_output_and_wide_box(ops):
    """the two turns of resample_u8_kernel that 256 -> 224 does not take: the column table's second turn (dim_out = 260 > 256 threads:
    columns 256 .. 259) and the lanes' second turn over a staged row's 16-byte pieces (a box 340 columns wide spans 1020 bytes and, with
    its start rounded down to 16, up to 65 pieces; the whole 344-column image 66).  Bits of the model; rrcref.launch_rows: 16 rows"""
    rng = np.random.RandomState(344260)
    boxes = wide_boxes()
    src = rng.randint(0, 256, size=(len(boxes), WIDE_IN, WIDE_IN, 3), dtype=np.uint8)
    assert rrcref.launch_rows(WIDE_IN, WIDE_OUT) == 16
    out, front, back = run_resample(ops, src, boxes, WIDE_OUT)
    check(out, rrcref.resample(src, boxes, WIDE_OUT))
    assert np.all(front == SENTINEL) and np.all(back == SENTINEL)


@pytest.mark.parametrize("dim_in,dim_out", [(256, 224), (37, 30), (32, 32)])
def test_a_dim_out_box_is_the_decode(ops, dim_in, dim_out):
    """h == w == dim_out: all weights are 0 and the output is mi_op_decode_u8's on (row0, col0, flip), bit for bit, on the device"""
    n = 9
    rng = np.random.RandomState(dim_in)
    src = rng.randint(0, 256, size=(n, dim_in, dim_in, 3), dtype=np.uint8)
    pl = augref.plan(augref.RANDOM, 1, 31, 0, 0, n, dim_in, dim_out)
    boxes = np.stack([pl[:, 0], pl[:, 1], np.full(n, dim_out), np.full(n, dim_out), pl[:, 2]], axis=1).astype(np.int32)
    a = ops.resample_u8(src, boxes, dim_out)
    b = ops.decode_u8(src, pl, dim_out)
    check(a, b)
    check(a, augref.decode(src, pl, dim_out))


def test_ops_resample_pads_like_decode(ops):
    rng = np.random.RandomState(2)
    src = rng.randint(0, 256, size=(2, 37, 37, 3), dtype=np.uint8)
    boxes = rrcref.plan(1, 3, 0, 0, 2, 37)
    out, pad = ops.resample_u8(src, boxes, 30, pad_floats=64, fill=SENTINEL)
    check(out, rrcref.resample(src, boxes, 30))
    assert pad.shape == (64,) and np.all(pad == SENTINEL)


def test_resample_refuses_an_unaligned_source(ops):
    src = ops.dev(np.zeros(64 * 64 * 3 + 16, np.uint8))
    bx = ops.dev(np.array([[0, 0, 64, 64, 0]], np.int32))
    out = ops.dev(shape=(1, 3, 32, 32))
    assert ops.L.mi_op_resample_u8(src.ptr + 4, bx.ptr, out.ptr, 1, 64, 32) == -1
    assert "16-byte" in ops.L.mi_last_error().decode()
    ops.L.mi_clear_error()
    assert ops.L.mi_op_resample_u8(src.ptr, bx.ptr, out.ptr, 1, 64, 32) == 0


def test_resample_refuses_an_image_too_wide_for_lds(ops):
    """the smallest dim_in at which the two source rows of ONE output row (+ the tables) exceed 64 KB, from the launcher's formula:
    -2 with a message, and nothing is launched (the output keeps its fill).  The box is 1 x 1 and the source has its full size."""
    D = 224
    dim_in = next(d for d in range(D, 16385) if rrcref.launch_rows(d, D) == 0)
    assert rrcref.launch_rows(dim_in - 1, D) == 1 and rrcref.lds_bytes(1, dim_in, D) > 65536 >= rrcref.lds_bytes(1, dim_in - 1, D)
    src = ops.dev(shape=(1, dim_in, dim_in, 3), dtype=np.uint8)
    bx = ops.dev(np.array([[0, 0, 1, 1, 0]], np.int32))
    out = ops.dev(np.full((1, 3, D, D), SENTINEL, np.float32))
    assert ops.L.mi_op_resample_u8(src.ptr, bx.ptr, out.ptr, 1, dim_in, D) == -2
    assert "LDS" in ops.L.mi_last_error().decode()
    ops.L.mi_clear_error()
    assert np.all(out.get() == SENTINEL)


# ---------------------------------------------------------------- the loader
DIN, DOUT, SEED = 40, synth.C1_DIMS["input"], 4242
SCALE, RATIO = (0.2, 1.0), (0.5, 2.0)  # not the defaults: the bounds must reach the plan


def expect(shards, sid, first_in_shard, n, per_shard, epoch, dim_in=DIN, dim_out=DOUT, scale=SCALE, ratio=RATIO):
    """(input, labels, boxes) of images [first_in_shard, + n) of shard sid"""
    img, lab, _ = shards[sid]
    sl = slice(first_in_shard, first_in_shard + n)
    bx = rrcref.plan(1, SEED, epoch, sid * per_shard + first_in_shard, n, dim_in, scale, ratio)
    return rrcref.resample(img[sl], bx, dim_out), lab[sl], bx


def rrc_source(tr, u8_dir, prefetch, dim_in=DIN, scale=SCALE, ratio=RATIO):
    tr.source_shards_u8(u8_dir, dim_in, augment="rrc", flip=True, seed=SEED, prefetch=prefetch, scale=scale, ratio=ratio)


def run_loader(u8_dir, shards, prefetch, per_shard=24, batch=4):
    """one epoch over both shards and a quarter of the next, full training steps between the loads"""
    tr = make_trainer(batch, per_shard, n_epochs=3)
    inputs, losses = [], []
    try:
        tr.L.mi_trainer_set_input_reset(tr.t, 1)
        rrc_source(tr, u8_dir, prefetch)
        per = per_shard // batch
        for epoch, steps in ((0, 2 * per), (1, 3)):
            for step in range(steps):
                tr.load_new_batch()
                assert tr.L.mi_batch_last_status(tr.c_batch) == 0
                sid, b = divmod(step, per)
                x, lab, bx = expect(shards, sid, b * batch, batch, per_shard, epoch)
                got = tr.activation("input")
                assert np.array_equal(tr.last_boxes(), bx), (epoch, step)
                assert np.array_equal(bits(got), bits(x)), (epoch, step)
                assert np.array_equal(tr.labels(), lab)
                assert tr.c_batch.contents.cur_shard_id == sid
                with pytest.raises(RuntimeError):
                    tr.last_plan()
                inputs.append(got)
                tr.forward()
                losses.append(tr.loss()[0])
                tr.backward()
                tr.update()
            tr.L.mi_trainer_end_epoch(tr.t, 0.0, 0.0, float(2 * per_shard))
            assert tr.t.contents.cur_epoch == epoch + 1
        tr.check()
    finally:
        tr.close()
    return inputs, losses


def test_loader_rrc_blocking_and_prefetched(tmp_path):
    shards, u8, _ = write_u8_shards(str(tmp_path), 2, 24, DIN, DOUT)
    xa, la = run_loader(u8, shards, False)
    xb, lb = run_loader(u8, shards, True)
    assert len(xa) == 15 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(xa, xb))
    assert la == lb and all(np.isfinite(la))
    assert not np.array_equal(bits(xa[0]), bits(xa[12]))  # batch 0 of shard 0 in epoch 0 and in epoch 1


def test_set_augment_rrc_is_for_u8_shards_only_and_checks_its_bounds(tmp_path):
    shards, u8, _ = write_u8_shards(str(tmp_path), 1, 8, DIN, DOUT)
    tr = make_trainer(4, 8)
    try:
        tr.source_synthetic()
        assert tr.L.mi_batch_set_augment_rrc(tr.c_batch, 1, 5, 0.08, 1.0, 0.75, 4 / 3) == -1
        assert "MI_SRC_SHARDS_U8" in tr.error()
        tr.L.mi_clear_error()
        with pytest.raises(RuntimeError):
            tr.last_boxes()
        with pytest.raises(RuntimeError):
            rrc_source(tr, u8, False, scale=(0.5, 0.25))
        assert tr.error() == ""
        rrc_source(tr, u8, False)
        with pytest.raises(RuntimeError):
            tr.last_boxes()  # nothing loaded yet
    finally:
        tr.close()


@pytest.mark.parametrize("prefetch", [False, True])
def test_rank_slices(tmp_path, prefetch):
    """world 2: the two ranks' batches are the halves of the world-1 batch of 2 N images, drawn at their GLOBAL indices; a ragged tail of
    4 of 20 images is skipped by both at the same step"""
    N, W, per_shard = 4, 2, 20
    shards, u8, _ = write_u8_shards(str(tmp_path), 2, per_shard, DIN, DOUT, seed=9)
    trs = []
    try:
        for r in range(W):
            tr = make_trainer(N, per_shard)
            rrc_source(tr, u8, prefetch)
            tr.L.mi_batch_set_rank_slice(tr.c_batch, r, W)
            trs.append(tr)
        per = per_shard // (W * N)
        for step in range(2 * per):
            sid, g = divmod(step, per)
            x, lab, bx = expect(shards, sid, g * W * N, W * N, per_shard, 0)  # the world-1 batch
            for r, tr in enumerate(trs):
                tr.load_new_batch()
                assert tr.L.mi_batch_last_status(tr.c_batch) == 0
                half = slice(r * N, (r + 1) * N)
                assert np.array_equal(tr.last_boxes(), bx[half]), (step, r)
                assert np.array_equal(bits(tr.activation("input")), bits(x[half])), (step, r)
                assert np.array_equal(tr.labels(), lab[half])
                assert tr.c_batch.contents.cur_shard_id == sid
                if prefetch:
                    tr.forward(); tr.backward(); tr.update()
    finally:
        for tr in trs:
            tr.close()


@pytest.mark.parametrize("prefetch", [False, True])
def test_a_resumed_run_sees_the_same_pixels(tmp_path, prefetch):
    per_shard, batch = 12, 4
    shards, u8, _ = write_u8_shards(str(tmp_path / "data"), 1, per_shard, DIN, DOUT, seed=11)
    root = str(tmp_path / "dumps")

    def fresh():
        tr = make_trainer(batch, per_shard, dump_dir="run", n_epochs=3)
        tr.L.mi_trainer_set_dump_root(tr.t, root.encode())
        rrc_source(tr, u8, prefetch)
        return tr

    a = fresh()
    try:
        for b in range(3):  # epoch 0: the whole shard
            a.load_new_batch()
            a.forward(); a.backward(); a.update()
        a.L.mi_trainer_end_epoch(a.t, 0.0, 0.0, float(per_shard))
        for b in range(2):
            a.load_new_batch()
            a.forward(); a.backward()
            if b == 0:
                a.update()
        a.L.dump_trainer(5, a.t, b"run")  # in the middle of step 2 of epoch 1: the next load is batch 2 of shard 0
        a.update()
        a.load_new_batch()
        want, want_boxes, want_lab = a.activation("input"), a.last_boxes(), a.labels()
        x, lab, bx = expect(shards, 0, 2 * batch, batch, per_shard, 1)
        assert np.array_equal(bits(want), bits(x)) and np.array_equal(want_boxes, bx)
    finally:
        a.close()

    b = fresh()  # seed, mode and bounds are not dumped: fresh() sets them again
    try:
        b.L.overwrite_trainer_hyperparams(b.t, 5, b"run")
        assert b.t.contents.init_loaded == 1 and b.t.contents.cur_epoch == 1 and b.c_batch.contents.cur_batch_in_shard == 2
        b.load_new_batch()
        assert b.L.mi_batch_last_status(b.c_batch) == 0
        assert np.array_equal(b.last_boxes(), want_boxes) and np.array_equal(b.labels(), want_lab)
        assert np.array_equal(bits(b.activation("input")), bits(want))
    finally:
        b.close()


@pytest.mark.parametrize("prefetch", [False, True])
def test_switching_back_to_random_reproduces_the_crop_path(tmp_path, prefetch):
    """rrc for two loads, then mi_batch_set_augment(RANDOM) on the same batch object: the next loads are the existing path's bits (a
    batch prefetched under rrc must not be taken), last_plan works again and last_boxes does not; and back once more"""
    from resnet_amd import binding as B
    per_shard, batch = 24, 4
    shards, u8, _ = write_u8_shards(str(tmp_path), 1, per_shard, DIN, DOUT, seed=5)
    img, lab, _ = shards[0]
    tr = make_trainer(batch, per_shard)
    try:
        rrc_source(tr, u8, prefetch)
        for b in range(2):
            tr.load_new_batch()
            assert np.array_equal(bits(tr.activation("input")), bits(expect(shards, 0, b * batch, batch, per_shard, 0)[0]))
            tr.forward(); tr.backward(); tr.update()
        assert tr.L.mi_batch_set_augment(tr.c_batch, B.MI_AUG_RANDOM, 1, SEED) == 0
        with pytest.raises(RuntimeError):
            tr.last_boxes()
        with pytest.raises(RuntimeError):
            tr.last_plan()  # the last load left boxes, not a plan
        for b in range(2, 4):
            tr.load_new_batch()
            assert tr.L.mi_batch_last_status(tr.c_batch) == 0
            pl = augref.plan(augref.RANDOM, 1, SEED, 0, b * batch, batch, DIN, DOUT)
            assert np.array_equal(tr.last_plan(), pl)
            assert np.array_equal(bits(tr.activation("input")), bits(augref.decode(img[b * batch:(b + 1) * batch], pl, DOUT))), b
            with pytest.raises(RuntimeError):
                tr.last_boxes()
            tr.forward(); tr.backward(); tr.update()
        assert tr.L.mi_batch_set_augment_rrc(tr.c_batch, 1, SEED, SCALE[0], SCALE[1], RATIO[0], RATIO[1]) == 0
        tr.load_new_batch()
        x, _, bx = expect(shards, 0, 4 * batch, batch, per_shard, 0)
        assert np.array_equal(tr.last_boxes(), bx) and np.array_equal(bits(tr.activation("input")), bits(x))
        tr.check()
    finally:
        tr.close()


def write_full_size_shard(root, per_shard, dim_in):
    """one uint8 shard of per_shard seeded images (no fp32 twin: 256 images of 224^2 floats are 150 MB)"""
    from resnet_amd import binding as B
    lib = B.load()
    rng = np.random.RandomState(21)
    n_classes, per_class = 4, 8
    data, u8 = os.path.join(root, "classes"), os.path.join(root, "u8")
    os.makedirs(data), os.makedirs(u8)
    classes = rng.randint(0, 256, size=(n_classes, per_class, dim_in, dim_in, 3), dtype=np.uint8)
    for c in range(n_classes):
        classes[c].tofile(os.path.join(data, "%08d.buffer" % c))
    rows = [(i % n_classes, (i // n_classes) % per_class, 0, 0) for i in range(per_shard)]
    csv = os.path.join(root, "000_images.csv")
    with open(csv, "w") as f:
        for r in rows:
            f.write("%03d,%04d,%02d,%02d\n" % r)
    assert lib.mi_build_shard_u8(csv.encode(), data.encode(), u8.encode(), 0, dim_in) == per_shard
    return [(np.stack([classes[c][k] for c, k, _, _ in rows]), np.array([r[0] for r in rows], np.int32), None)], u8


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_full_size_step(tmp_path, dtype):
    """ResNet-50 at 224^2, batch 256, from a 256^2 uint8 shard with the default bounds: one full step; the first and the last images
    of the batch are the model's"""
    from resnet_amd import binding as B
    per_shard = batch = 256
    shards, u8 = write_full_size_shard(str(tmp_path), per_shard, 256)
    tr = make_trainer(batch, per_shard, dims=synth.R50_DIMS)
    try:
        if dtype == "bf16":
            tr.set_dtype(B.MI_DTYPE_BF16)
        tr.source_shards_u8(u8, 256, augment="rrc", flip=True, seed=SEED)
        tr.load_new_batch()
        assert tr.L.mi_batch_last_status(tr.c_batch) == 0
        bx = rrcref.plan(1, SEED, 0, 0, batch, 256)
        assert np.array_equal(tr.last_boxes(), bx) and np.array_equal(tr.labels(), shards[0][1])
        got = tr.activation("input")
        for sl in (slice(0, 4), slice(batch - 4, batch)):
            check(got[sl], rrcref.resample(shards[0][0][sl], bx[sl], 224))
        tr.forward()
        loss = tr.loss()[0]
        tr.backward()
        tr.update()
        assert tr.check_errors() == 0
        assert tr.error() == ""
        assert np.isfinite(loss)
    finally:
        tr.close()
