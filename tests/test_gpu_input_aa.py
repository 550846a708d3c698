"""The antialiased resize on the device (include/resnet_mi.h, "antialiased resize"): resample_aa_u8_kernel (kernels_input.hip) against
the numpy model (tests/aaref.py, itself held against Pillow by tests/test_input_aa.py), the loader with antialias on, and the resized
evaluation.  Tiny shapes; everything is compared bit for bit."""
import numpy as np
import pytest

import aaref
import rrcref
import synth
from test_gpu_input_rrc import DIN, DOUT, SEED, check, expect
from test_gpu_input_u8 import SENTINEL, bits, make_trainer, write_u8_shards

pytestmark = pytest.mark.gpu

# (dim_in, virt, dim_out, window): one output pixel; odd sizes with a scalar tail; dim_out % 4 == 0; an upscale; no scaling at all;
# a window inside the resized image, square and not
OLD_CASES = [(8, 1, 1, 0), (9, 4, 4, 0), (33, 7, 7, 0), (32, 8, 8, 0), (16, 24, 24, 0), (40, 40, 40, 0), (64, 58, 52, 3), (64, 29, 22, (0, 7))]
# the loop turns and launcher branches that OLD_CASES never take, each at the smallest shape that takes it ("Suite
# sensitivity"); the numbers are the launcher's, from aaref.launch_rows / aaref.lds_bytes, and test_new_cases_are_on_their_branches
# holds them so that a launcher change which moves a case off its branch fails loudly.  AA_THREADS = 256, Q = dim_out / 4:
# (100, 68, 68, 0)    the row pass `for (i = tid; i < nrows * Q; i += 256)` takes a second turn: R = 16, 16 x 17 = 272 items; D = 64
#                     gives exactly 256
# (300, 260, 260, 0)  the table fill `for (i = tid; i < D; i += 256)` takes a second turn (the smallest D % 4 == 0 past 256); 1040 row
#                     items: 5 turns
# (200, 24, 24, 0)    1 < R < 16 with a ragged last workgroup: R = 9, workgroups of 9, 9 and 6 rows; 19-tap rows
# (294, 100, 100, 0)  1 < R < 16 together with a second row-pass turn: R = 15, 15 x 25 = 375 items; the smallest dim_in for D = 100
# No case stages a row of more than 64 16-byte pieces (the lanes' second turn `for (c = tid & 63; c < pieces; c += 64)`, boxes of 337
# columns and more): test_refuses_an_image_too_wide_for_lds does, with 89 pieces, and is the killer of that turn's mutant
NEW_CASES = {(100, 68, 68, 0): dict(R=16, items=272, ks=5, lds=15976, second_turn=True),
             (300, 260, 260, 0): dict(R=16, items=1040, ks=5, lds=43596, second_turn=True, wide_table=True),
             (200, 24, 24, 0): dict(R=9, items=54, ks=19, lds=61944, groups=[9, 9, 6], lower_R=True),
             (294, 100, 100, 0): dict(R=15, items=375, ks=7, lds=63532, second_turn=True, lower_R=True)}
CASES = OLD_CASES + list(NEW_CASES)
N = 3
AA_THREADS = 256


def corner_box(d):
    small = max(d // 3, 1)
    return (d - small, d - min(7, d), small, min(7, d), 0)


def box_sets(d, rng):
    """batches of N boxes; the LAST image's box of the first set is flush with the bottom-right corner: its last span ends with the batch"""
    h, w = rng.randint(1, d + 1, size=2)
    return {
        "whole+corner": [(0, 0, d, d, 0), (0, 0, d, d, 1), corner_box(d)],
        "thin": [(0, 0, 1, 1, 0), (min(5, d - 1), 0, 1, d, 1), (0, min(7, d - 1), d, 1, 0)],
        "thin, flipped": [(d - 1, d - 1, 1, 1, 1), (d - 1, 0, 1, d, 0), (0, d - 1, d, 1, 1)],
        "clamped": [(-5, d + 3, 0, 900, 7), (1000, -1000, 2 * d, 3, 1), (2, 2, -4, -4, 0)],
        "mixed": [(rng.randint(0, d - h + 1), rng.randint(0, d - w + 1), h, w, 1), (0, 0, d, max(d // 4, 1), 0), (0, 0, max(d // 5, 1), d, 1)],
    }


_SRC = {}


def source(d):
    if d not in _SRC:
        _SRC[d] = np.random.RandomState(1000 + d).randint(0, 256, size=(N, d, d, 3), dtype=np.uint8)
    return _SRC[d]


def run_aa(ops, src, boxes, D, virt, win, front=1024, back=1024, rc_want=0):
    """mi_op_resample_aa_u8 into the middle of a pre-filled buffer -> (images, the floats in front, the floats behind)"""
    n, dim_in = src.shape[0], src.shape[1]
    wr, wc = (win, win) if np.isscalar(win) else win
    total = n * 3 * D * D
    dsrc, dbox = ops.dev(src), ops.dev(np.ascontiguousarray(boxes, np.int32))
    dout = ops.dev(np.full(front + total + back, SENTINEL, np.float32))
    rc = ops.L.mi_op_resample_aa_u8(dsrc.ptr, dbox.ptr, dout.ptr + 4 * front, n, dim_in, D, virt, wr, wc)
    assert rc == rc_want, ops.L.mi_last_error().decode()
    out = dout.get()
    return out[front:front + total].reshape(n, 3, D, D), out[:front], out[front + total:]


def test_new_cases_are_on_their_branches():
    """host arithmetic only (tests/test_input_aa.py runs it without a device as well): the launcher's answer for every new case is the
    one it was chosen for, and no old case reaches any of these branches"""
    for (dim_in, virt, D, win), want in NEW_CASES.items():
        R = aaref.launch_rows(dim_in, D, virt)
        assert (R, R * (D // 4), aaref.ksize(dim_in, virt), aaref.lds_bytes(R, dim_in, D, virt)) == (want["R"], want["items"], want["ks"], want["lds"])
        assert aaref.lds_bytes(R, dim_in, D, virt) <= aaref.AA_LDS_MAX
        assert (R * (D // 4) > AA_THREADS) == bool(want.get("second_turn")) and (D > AA_THREADS) == bool(want.get("wide_table"))
        assert (1 < R < aaref.AA_ROWS) == bool(want.get("lower_R"))
        if want.get("lower_R"):  # R is lowered because R + 1 does not fit, not because dim_out is small
            assert D > R and aaref.lds_bytes(R + 1, dim_in, D, virt) > aaref.AA_LDS_MAX
        if "groups" in want:
            assert [min(R, D - h0) for h0 in range(0, D, R)] == want["groups"]
    assert aaref.launch_rows(100, 64, 64) * (64 // 4) == AA_THREADS  # D = 64: exactly one turn; 68 is the next multiple of 4
    assert all(aaref.launch_rows(d, 100, 100) == 16 for d in range(100, 294))  # 294: the smallest dim_in with R < 16 at D = 100
    for dim_in, virt, D, win in OLD_CASES:
        R = aaref.launch_rows(dim_in, D, virt)
        assert R == min(16, D) and R * (D // 4) <= AA_THREADS and D <= AA_THREADS
    assert all((3 * c[0] + 30) >> 4 <= 64 for c in CASES) and (3 * (lds_limit_inputs()[1] - 1) + 30) >> 4 > 64


# ---------------------------------------------------------------- the kernel on its own
@pytest.mark.parametrize("dim_in,virt,dim_out,win", CASES)
def test_sweep(ops, dim_in, virt, dim_out, win):
    rng = np.random.RandomState(dim_in * 100 + virt)
    src = source(dim_in)
    for name, boxes in box_sets(dim_in, rng).items():
        boxes = np.array(boxes, np.int32)
        cl = np.array([rrcref.clamp_box(b, dim_in) for b in boxes])
        if name == "whole+corner":
            assert np.array_equal(cl[-1, :2] + cl[-1, 2:4], (dim_in, dim_in))
        if name == "clamped":
            assert not np.array_equal(cl, boxes)
        out, front, back = run_aa(ops, src, boxes, dim_out, virt, win)
        ref = aaref.resample(src, boxes, dim_out, virt, win)
        bad = np.argwhere(bits(out) != bits(ref))
        assert bad.size == 0, "%s: first mismatch at (n, d, h, w) = %s of %d" % (name, bad[0], len(bad))
        assert np.all(front == SENTINEL) and np.all(back == SENTINEL), name


@pytest.mark.parametrize("dim_in,virt,dim_out,win", [(32, 8, 8, 0), (64, 58, 52, 3)])
def test_into_an_output_one_float_off_alignment(ops, dim_in, virt, dim_out, win):
    """dim_out % 4 == 0 but out 4 bytes off a 16-byte boundary: the element-wise stores; the floats around the images keep their fill"""
    src = source(dim_in)
    boxes = np.array(box_sets(dim_in, np.random.RandomState(3))["whole+corner"], np.int32)
    out, front, back = run_aa(ops, src, boxes, dim_out, virt, win, front=1021, back=1027)
    check(out, aaref.resample(src, boxes, dim_out, virt, win))
    assert np.all(front == SENTINEL) and np.all(back == SENTINEL)
    got, pad = ops.resample_aa_u8(src, boxes, dim_out, virt, win, pad_floats=64, fill=SENTINEL)
    check(got, out)
    assert pad.shape == (64,) and np.all(pad == SENTINEL)


@pytest.mark.parametrize("dim_in,virt,dim_out,win", CASES)
def test_corner_case_under_the_red_zone(ops, dim_in, virt, dim_out, win):
    """every allocation between two 4096-byte zones of 0xFF: the box that ends with the batch, and none of the zones is written"""
    L = ops.L
    src = source(dim_in)
    boxes = np.array(box_sets(dim_in, np.random.RandomState(3))["whole+corner"], np.int32)
    assert L.mi_debug_redzone(4096, 0xFF) == 0
    try:
        out = ops.resample_aa_u8(src, boxes, dim_out, virt, win)
        assert L.mi_debug_redzone_check() == 0, L.mi_last_error().decode()
    finally:
        L.mi_debug_redzone(0, 0)
    check(out, aaref.resample(src, boxes, dim_out, virt, win))


@pytest.mark.parametrize("dim_in,virt,dim_out,win", CASES)
def test_same_bits_with_lds_full_of_ones(ops, dim_in, virt, dim_out, win):
    """every LDS word 0xFFFFFFFF before the launch: a byte or a coefficient read that the workgroup did not write would show"""
    L = ops.L
    src = source(dim_in)
    sets = box_sets(dim_in, np.random.RandomState(dim_in * 100 + virt))
    assert L.mi_debug_lds_fill_mode(1, 0xFFFFFFFF) == 0, L.mi_last_error()
    try:
        outs = {k: ops.resample_aa_u8(src, np.array(b, np.int32), dim_out, virt, win) for k, b in sets.items()}
        assert L.mi_debug_lds_fills() >= len(sets)
    finally:
        L.mi_debug_lds_fill_mode(0, 0)
    for k, b in sets.items():
        check(outs[k], aaref.resample(src, np.array(b, np.int32), dim_out, virt, win))


def test_a_box_of_the_output_size_is_the_decode(ops):
    """h = w = virt = dim_out: both passes hand the bytes through -- mi_op_decode_u8's bits on (row0, col0, flip)"""
    import augref
    for dim_in, D in ((37, 30), (40, 32), (32, 32)):
        n = 5
        src = np.random.RandomState(dim_in).randint(0, 256, size=(n, dim_in, dim_in, 3), dtype=np.uint8)
        pl = augref.plan(augref.RANDOM, 1, 31, 0, 0, n, dim_in, D)
        boxes = np.stack([pl[:, 0], pl[:, 1], np.full(n, D), np.full(n, D), pl[:, 2]], axis=1).astype(np.int32)
        a = ops.resample_aa_u8(src, boxes, D)
        check(a, ops.decode_u8(src, pl, D))
        check(a, augref.decode(src, pl, D))


def test_an_upscale_is_the_models_not_the_gathers(ops):
    """a box smaller than the output: Pillow's three-tap table, by design not resample_u8's convention"""
    dim_in, D = 40, 32
    src = source(dim_in)
    boxes = np.array([(3, 4, 9, 11, 0), (20, 1, 13, 7, 1), (0, 0, 5, 5, 1)], np.int32)
    a = ops.resample_aa_u8(src, boxes, D)
    check(a, aaref.resample(src, boxes, D))
    assert not np.array_equal(bits(a), bits(ops.resample_u8(src, boxes, D)))


def test_refusals_write_nothing(ops):
    L = ops.L
    src = ops.dev(np.zeros(64 * 64 * 3 + 16, np.uint8))
    bx = ops.dev(np.array([[0, 0, 64, 64, 0]], np.int32))
    out = ops.dev(np.full((1, 3, 32, 32), SENTINEL, np.float32))
    assert L.mi_op_resample_aa_u8(src.ptr + 4, bx.ptr, out.ptr, 1, 64, 32, 32, 0, 0) == -1
    assert "16-byte" in L.mi_last_error().decode()
    L.mi_clear_error()
    for virt, wr, wc in ((32, 1, 0), (32, 0, 1), (40, 9, 0), (40, 0, -1), (31, 0, 0)):
        assert L.mi_op_resample_aa_u8(src.ptr, bx.ptr, out.ptr, 1, 64, 32, virt, wr, wc) == -1, (virt, wr, wc)
        assert "window" in L.mi_last_error().decode()
        L.mi_clear_error()
    for n, dim_in, D, virt in ((0, 64, 32, 32), (65536, 64, 32, 32), (1, 0, 32, 32), (1, 16385, 32, 32), (1, 64, 0, 32), (1, 64, 32, 16385)):
        assert L.mi_op_resample_aa_u8(src.ptr, bx.ptr, out.ptr, n, dim_in, D, virt, 0, 0) == -1, (n, dim_in, D, virt)
        L.mi_clear_error()
    assert np.all(out.get() == SENTINEL)
    assert L.mi_op_resample_aa_u8(src.ptr, bx.ptr, out.ptr, 1, 64, 32, 40, 8, 8) == 0
    assert not np.any(out.get() == SENTINEL)


def lds_limit_inputs():
    """(D, the smallest dim_in the launcher refuses at D, one image a pixel smaller, its whole box flipped)"""
    D = 24
    dim_in = next(d for d in range(D, 16385) if aaref.launch_rows(d, D, D) == 0)
    img = np.random.RandomState(5).randint(0, 256, size=(1, dim_in - 1, dim_in - 1, 3), dtype=np.uint8)
    return D, dim_in, img, np.array([[0, 0, dim_in - 1, dim_in - 1, 1]], np.int32)


def test_refuses_an_image_too_wide_for_lds(ops):
    """the smallest dim_in at which the tables and source rows of ONE output row exceed 64 KB, from the launcher's formula: -2 with a
    message, nothing launched; one pixel less runs"""
    D, dim_in, img, whole = lds_limit_inputs()
    assert aaref.launch_rows(dim_in - 1, D, D) == 1 and aaref.lds_bytes(1, dim_in, D, D) > 65536 >= aaref.lds_bytes(1, dim_in - 1, D, D)
    src = ops.dev(shape=(1, dim_in, dim_in, 3), dtype=np.uint8)
    bx = ops.dev(np.array([[0, 0, 1, 1, 0]], np.int32))
    out = ops.dev(np.full((1, 3, D, D), SENTINEL, np.float32))
    assert ops.L.mi_op_resample_aa_u8(src.ptr, bx.ptr, out.ptr, 1, dim_in, D, D, 0, 0) == -2
    assert "LDS" in ops.L.mi_last_error().decode()
    ops.L.mi_clear_error()
    assert np.all(out.get() == SENTINEL)
    check(ops.resample_aa_u8(img, whole, D), aaref.resample(img, whole, D))  # R = 1, the most taps that fit


# ---------------------------------------------------------------- the loader
def test_loader_antialias_blocking_and_prefetched_and_off_again(tmp_path):
    """two shards of 12 images, 40 -> 32, batch 4, rrc with flips: with antialias on Batch.images is the model on last_boxes(), blocking
    and prefetched, with full steps between the loads; switched off on the same batch object the next loads are the bilinear bits"""
    per_shard, batch = 12, 4
    shards, u8, _ = write_u8_shards(str(tmp_path), 2, per_shard, DIN, DOUT)
    per = per_shard // batch
    runs = []
    for prefetch in (False, True):
        tr = make_trainer(batch, per_shard)
        got = []
        try:
            tr.source_shards_u8(u8, DIN, augment="rrc", flip=True, seed=SEED, prefetch=prefetch, scale=(0.2, 1.0), ratio=(0.5, 2.0), antialias=True)
            for step in range(per + 1):
                tr.load_new_batch()
                assert tr.L.mi_batch_last_status(tr.c_batch) == 0
                sid, b = divmod(step, per)
                _, lab, bx = expect(shards, sid, b * batch, batch, per_shard, 0)
                assert np.array_equal(tr.last_boxes(), bx) and np.array_equal(tr.labels(), lab), step
                x = tr.activation("input")
                check(x, aaref.resample(shards[sid][0][b * batch:(b + 1) * batch], bx, DOUT))
                got.append(x)
                tr.forward(); tr.backward(); tr.update()
            assert tr.L.mi_batch_set_antialias(tr.c_batch, 0) == 0  # a batch prefetched with it on must not be taken
            for step in range(per + 1, per + 3):
                tr.load_new_batch()
                sid, b = divmod(step, per)
                x, _, bx = expect(shards, sid, b * batch, batch, per_shard, 0)
                assert np.array_equal(tr.last_boxes(), bx)
                check(tr.activation("input"), x)
                tr.forward(); tr.backward(); tr.update()
            tr.check()
        finally:
            tr.close()
        runs.append(got)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(*runs))


def test_set_antialias_is_for_u8_shards_only():
    tr = make_trainer(4, 8)
    try:
        tr.source_synthetic()
        assert tr.L.mi_batch_set_antialias(tr.c_batch, 1) == -1
        assert "MI_SRC_SHARDS_U8" in tr.error()
        tr.L.mi_clear_error()
    finally:
        tr.close()


# ---------------------------------------------------------------- evaluation
def eval_trainer(batch):
    from resnet_amd import Trainer
    from resnet_amd import binding as B
    dims = synth.C1_DIMS
    tr = Trainer(dims, batch)
    if tr.L.mi_device_count() < 1:
        pytest.fail("no HIP device: this test must run on the MI355X box")
    tr.set_params(synth.make_params(dims, perturb_bn=True))
    tr.source_host(B.MI_LAYOUT_NHWC)
    tr.track_running_stats(0.1)
    im, lab = synth.make_batch(dims, batch, step=0)
    tr.fill_host_batch(im, lab)
    tr.load_new_batch()
    tr.forward()
    tr.check()
    return tr


@pytest.mark.parametrize("ema", [False, True])
def test_evaluate_u8_resized(ema):
    """a ragged last batch (2 N + 3 images).  resize == dim_in: mi_trainer_eval_u8's records in every field; resize = r: the eval pass fed
    the model's images -- whole image -> r x r, the centre window at (r - input) / 2; down- and upscaling, an odd margin"""
    dims, N, dim_in = synth.C1_DIMS, 4, 40
    D = dims["input"]
    n = 2 * N + 3
    rng = np.random.RandomState(78)
    images = rng.randint(0, 256, size=(n, dim_in, dim_in, 3)).astype(np.uint8)
    labels = rng.randint(0, dims["output"], size=n).astype(np.int32)
    tr = eval_trainer(N)
    try:
        if ema:
            tr.set_ema(0.5)
            tr.backward(); tr.update()  # the average now differs from the weights
            tr.eval_use_ema(True)
        plain = tr.evaluate_u8(images, labels, dim_in, topk=5)
        same = tr.evaluate_u8(images, labels, dim_in, topk=5, resize=dim_in)
        assert np.float64(same["loss_sum"]).tobytes() == np.float64(plain["loss_sum"]).tobytes() and same == plain
        whole = np.tile(np.array([0, 0, dim_in, dim_in, 0], np.int32), (n, 1))
        seen = [plain]
        for r in (D + 5, D, 48):
            x = aaref.resample(images, whole, D, r, (r - D) // 2)
            tr.eval_metrics(reset=True)
            for at in range(0, n, N):
                tr.eval_forward(x[at:at + N], labels[at:at + N])
            hand = tr.eval_metrics()[1]
            got = tr.evaluate_u8(images, labels, dim_in, topk=5, resize=r)
            assert got["rows"] == n and got["batches"] == 3
            assert np.float64(got["loss_sum"]).tobytes() == np.float64(hand["loss_sum"]).tobytes(), (r, got, hand)
            assert got == hand
            seen.append(got)
        assert len({s["loss_sum"] for s in seen}) == len(seen)  # every size is another set of pixels
        with pytest.raises(RuntimeError):
            tr.evaluate_u8(images, labels, dim_in, resize=D - 1)
        tr.L.mi_clear_error()
        assert tr.evaluate_u8(images, labels, dim_in, topk=5) == plain
        tr.check()
    finally:
        tr.close()
