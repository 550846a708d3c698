"""The host side of the random-resized crop (include/resnet_mi.h, "random-resized crop"): the box plan mi_augment_plan_rrc against its
math / numpy restatement (tests/rrcref.py), and the resample model anchored to the decode model and, through it, to the fixture the
REFERENCE binary wrote (tests/golden/shard_ref_golden.npz).  CPU only: integers and exact floats."""
import hashlib
import os

import numpy as np
import pytest

import augref
import rrcref
from test_input_u8 import build_u8
from test_shards import DIM_IN, DIM_OUT, GOLD, ROWS


def c_plan(flip, seed, epoch, first, n, dim_in, scale=rrcref.SCALE, ratio=rrcref.RATIO):
    from resnet_amd import binding as B
    lib = B.load()
    out = np.full((max(n, 0), 5), -7, np.int32)
    rc = lib.mi_augment_plan_rrc(flip, seed, epoch, first, n, dim_in, scale[0], scale[1], ratio[0], ratio[1], out.ctypes.data)
    return rc, out


def inside(p, dim_in):
    return (p[:, 2:4].min() >= 1 and np.all(p[:, 0] >= 0) and np.all(p[:, 1] >= 0) and np.all(p[:, 0] + p[:, 2] <= dim_in)
            and np.all(p[:, 1] + p[:, 3] <= dim_in))


@pytest.mark.parametrize("dim_in", [256, 37])
def test_plan_matches_the_model(dim_in):
    n = 4096
    for seed, epoch, first in ((0, 0, 0), (7, 1, 4096), (2 ** 63 + 5, 5, 2 ** 31 + 17), (1234, 2, 3 * 2 ** 33)):
        for flip in (0, 1):
            rc, got = c_plan(flip, seed, epoch, first, n, dim_in)
            ref = rrcref.plan(flip, seed, epoch, first, n, dim_in)
            bad = np.argwhere(np.any(got != ref, axis=1))
            assert rc == 0 and bad.size == 0, (seed, epoch, first, flip, bad[:1], got[bad[:1]], ref[bad[:1]])
            assert inside(got, dim_in)
            assert flip or not got[:, 4].any()
    # other bounds than the defaults, narrow and wide
    for scale, ratio in (((0.25, 0.5), (0.5, 2.0)), ((1.0, 1.0), (1.0, 1.0)), ((0.001, 0.01), (0.1, 10.0)), ((0.9, 1.7), (0.75, 4 / 3))):
        rc, got = c_plan(1, 99, 3, 12345, 512, dim_in, scale, ratio)
        assert rc == 0 and np.array_equal(got, rrcref.plan(1, 99, 3, 12345, 512, dim_in, scale, ratio)), (scale, ratio)
        assert inside(got, dim_in)


def test_plan_depends_on_the_global_index_epoch_and_seed_only():
    _, a = c_plan(1, 7, 2, 100, 64, 256)
    for k in (1, 16, 63):
        _, b = c_plan(1, 7, 2, 100 + k, 64 - k, 256)
        assert np.array_equal(a[k:], b)
    _, e = c_plan(1, 7, 3, 100, 64, 256)
    _, s = c_plan(1, 8, 2, 100, 64, 256)
    assert not np.array_equal(a, e) and not np.array_equal(a, s)
    assert np.mean(np.all(a[:, :4] == e[:, :4], axis=1)) < 0.1 and np.mean(np.all(a[:, :4] == s[:, :4], axis=1)) < 0.1
    assert c_plan(1, 7, 2, 100, 0, 256)[0] == 0  # nothing to do is no error


@pytest.mark.parametrize("dim_in", [256, 37])
def test_fallback_is_deterministic(dim_in):
    """an area of 4 images fits at no allowed ratio below 4 (w = 2 dim_in sqrt(ratio), h = 2 dim_in / sqrt(ratio)): all ten tries fail"""
    n = 64
    rc, p = c_plan(1, 5, 0, 0, n, dim_in, (4.0, 4.0), (3 / 4, 4 / 3))
    assert rc == 0 and np.all(p[:, :4] == (0, 0, dim_in, dim_in))
    assert set(p[:, 4]) == {0, 1}  # the flip is drawn all the same
    rc, p = c_plan(0, 5, 0, 0, n, dim_in, (4.0, 4.0), (2.0, 3.0))
    h = round(dim_in / 2)
    assert rc == 0 and np.all(p == ((dim_in - h) // 2, 0, h, dim_in, 0))
    rc, p = c_plan(0, 5, 0, 0, n, dim_in, (4.0, 4.0), (0.25, 0.5))
    w = round(dim_in * 0.5)
    assert rc == 0 and np.all(p == (0, (dim_in - w) // 2, dim_in, w, 0))
    for scale, ratio in (((4.0, 4.0), (3 / 4, 4 / 3)), ((4.0, 4.0), (2.0, 3.0)), ((4.0, 4.0), (0.25, 0.5))):
        assert np.array_equal(c_plan(1, 5, 0, 0, n, dim_in, scale, ratio)[1], rrcref.plan(1, 5, 0, 0, n, dim_in, scale, ratio))


def test_default_parameters_flip_and_scale_both_ways():
    """4096 rows: both flip values, and box sides below and above dim_out = 224 (the kernel scales up and down).  A fair coin misses a
    value in 4096 draws with probability 2^-4095; the sides: an area share below 0.08 + 0.92 / 4 already puts the geometric mean of the
    sides under 0.56 * 256 = 143, a share above 0.9 at ratio ~ 1 puts both above 224"""
    _, p = c_plan(1, 1234, 0, 0, 4096, 256)
    assert set(p[:, 4]) == {0, 1} and 0.46 <= p[:, 4].mean() <= 0.54
    sides = p[:, 2:4]
    assert (sides < 224).any() and (sides > 224).any()
    assert (sides.max(axis=1) < 224).any() and (sides.min(axis=1) > 224).any()
    assert sides.min() >= 1 and sides.max() <= 256


def test_plan_error_returns():
    from resnet_amd import binding as B
    lib = B.load()
    ok = dict(n=4, dim_in=256, scale=(0.08, 1.0), ratio=(0.75, 4 / 3))
    for bad in (dict(n=-1), dict(dim_in=0), dict(scale=(0.0, 1.0)), dict(scale=(-0.5, 1.0)), dict(ratio=(0.0, 1.0)), dict(ratio=(-1.0, 1.0)),
                dict(scale=(0.5, 0.4)), dict(ratio=(1.5, 1.0)), dict(scale=(float("nan"), 1.0))):
        a = dict(ok, **bad)
        lib.mi_clear_error()
        assert c_plan(1, 0, 0, 0, a["n"], a["dim_in"], a["scale"], a["ratio"])[0] == -1, bad
        assert "mi_augment_plan_rrc" in lib.mi_last_error().decode()
    lib.mi_clear_error()
    assert c_plan(1, 0, 0, 0, 4, 256)[0] == 0
    # the old entry point keeps refusing mode 3
    out = np.zeros((4, 3), np.int32)
    assert lib.mi_augment_plan(B.MI_AUG_RRC, 0, 0, 0, 0, 4, 256, 224, None, out.ctypes.data) == -1
    lib.mi_clear_error()


def test_resample_model_on_a_dim_out_box_is_the_decode():
    rng = np.random.RandomState(3)
    for dim_in, dim_out in ((40, 33), (37, 30), (32, 32), (64, 48)):
        n = 6
        src = rng.randint(0, 256, size=(n, dim_in, dim_in, 3), dtype=np.uint8)
        pl = augref.plan(augref.RANDOM, 1, 11, 0, 0, n, dim_in, dim_out)
        boxes = np.stack([pl[:, 0], pl[:, 1], np.full(n, dim_out), np.full(n, dim_out), pl[:, 2]], axis=1).astype(np.int32)
        assert np.array_equal(rrcref.resample(src, boxes, dim_out).view(np.uint32), augref.decode(src, pl, dim_out).view(np.uint32))


def test_resample_model_reproduces_the_reference_fixture(tmp_path):
    """the crops of the fixture as dim_out-sized boxes: the fp32 shard the REFERENCE binary wrote"""
    img, lab, crops, _ = build_u8(str(tmp_path))
    n = len(ROWS)
    boxes = np.concatenate([crops, np.full((n, 2), DIM_OUT), np.zeros((n, 1))], axis=1).astype(np.int32)
    out = rrcref.resample(img, boxes, DIM_OUT).ravel()
    gold = np.load(os.path.join(GOLD, "shard_ref_golden.npz"))
    assert out.size == int(gold["n_floats"])
    assert np.array_equal(out[:64].view(np.uint32), gold["head"].view(np.uint32))
    assert np.array_equal(out[-64:].view(np.uint32), gold["tail"].view(np.uint32))
    assert hashlib.sha256(out.tobytes()).hexdigest() == str(gold["sha256"])


def test_resample_model_properties():
    """a constant image stays constant at every scale; a whole-image box of an image that is linear in x stays monotonic; the flip
    mirrors the columns; an out-of-range box is its clamped box"""
    dim_in, D = 40, 33
    src = np.full((1, dim_in, dim_in, 3), 77, np.uint8)
    for b in ((0, 0, 1, 1, 0), (3, 5, 7, 31, 1), (0, 0, 40, 40, 0), (10, 10, 33, 33, 0)):
        out = rrcref.resample(src, np.array([b], np.int32), D)
        for d in range(3):
            assert np.all(out[0, d] == np.float32(77.0 - augref.MEAN_OF_SRC[2 - d]))
    ramp = np.broadcast_to((np.arange(dim_in) * 6)[None, None, :, None], (1, dim_in, dim_in, 3)).astype(np.uint8)
    a = rrcref.resample(ramp, np.array([(0, 0, 40, 40, 0)], np.int32), D)
    f = rrcref.resample(ramp, np.array([(0, 0, 40, 40, 1)], np.int32), D)
    assert np.all(np.diff(a[0, 0], axis=1) >= 0) and np.all(a[0, 0] == a[0, 0, :1])
    assert np.array_equal(f, a[:, :, :, ::-1])
    rng = np.random.RandomState(1)
    src = rng.randint(0, 256, size=(1, dim_in, dim_in, 3), dtype=np.uint8)
    assert np.array_equal(rrcref.resample(src, np.array([(-5, 38, 0, 900, 7)], np.int32), D),
                          rrcref.resample(src, np.array([(0, 0, 1, 40, 1)], np.int32), D))
    assert rrcref.clamp_box((39, -3, 20, 50, 0), dim_in) == (20, 0, 20, 40, 0)


def test_launcher_formula():
    """the row counts the GPU tests rely on: 16 output rows per workgroup at the sizes of the sweep, fewer for wide images, none at
    all beyond the size test_gpu_input_rrc refuses"""
    for di, do in ((256, 224), (257, 224), (37, 30), (40, 33), (32, 32)):
        assert rrcref.launch_rows(di, do) == min(16, do)
    assert 1 <= rrcref.launch_rows(2048, 224) < 16
    assert rrcref.launch_rows(16384, 224) == 0
