"""The host side of the uint8 input path (include/resnet_mi.h, "uint8 shards"): the shard writer mi_build_shard_u8, the numpy model
of the decode against the fixture the REFERENCE binary wrote (tests/golden/shard_ref_golden.npz), and the augmentation plan
mi_augment_plan against its numpy restatement (tests/augref.py).  CPU only: bytes, integers and exact floats."""
import ctypes as C
import hashlib
import os

import numpy as np

import augref
from test_shards import DIM_IN, DIM_OUT, GOLD, N_CLASSES, ROWS, class_bytes, write_inputs


def build_u8(tmp):
    """mi_build_shard_u8 on the synthetic class files of test_shards -> (images_u8, labels, crops, out_dir)"""
    from resnet_amd import binding as B
    lib = B.load()
    part, data = write_inputs(os.path.join(tmp, "in"))
    out = os.path.join(tmp, "out_u8")
    os.makedirs(out)
    rc = lib.mi_build_shard_u8(os.path.join(part, "000_images.csv").encode(), data.encode(), out.encode(), 0, DIM_IN)
    assert rc == len(ROWS)
    img = np.fromfile(os.path.join(out, "000.images_u8"), np.uint8).reshape(len(ROWS), DIM_IN, DIM_IN, 3)
    return img, np.fromfile(os.path.join(out, "000.labels"), np.int32), np.fromfile(os.path.join(out, "000.crops"), np.int32).reshape(-1, 2), out


def c_plan(mode, flip, seed, epoch, first, n, dim_in, dim_out, fixed=None):
    from resnet_amd import binding as B
    lib = B.load()
    out = np.full((n, 3), -7, np.int32)
    fx = np.ascontiguousarray(fixed, np.int32) if fixed is not None else None
    rc = lib.mi_augment_plan(mode, flip, seed, epoch, first, n, dim_in, dim_out, fx.ctypes.data if fx is not None else None, out.ctypes.data)
    return rc, out


def test_writer_keeps_whole_images_crops_and_labels(tmp_path):
    from resnet_amd import binding as B
    lib = B.load()
    img, lab, crops, _ = build_u8(str(tmp_path))
    classes = [class_bytes(c) for c in range(N_CLASSES)]
    assert np.array_equal(img, np.stack([classes[c][n] for c, n, _, _ in ROWS]))  # whole images, B,G,R interleaving kept
    assert np.array_equal(crops, np.array([(r, s) for _, _, r, s in ROWS], np.int32))
    # the labels file is mi_build_shard's
    part = os.path.join(str(tmp_path), "in", "data/vision/imagenet/2012/train_data_partioning", "000_images.csv")
    data = os.path.join(str(tmp_path), "in", "data/vision/imagenet/2012/train_data")
    f32 = tmp_path / "out_f32"
    f32.mkdir()
    assert lib.mi_build_shard(part.encode(), data.encode(), str(f32).encode(), 0, DIM_IN, DIM_OUT, B.MI_LAYOUT_NCHW) == len(ROWS)
    assert np.array_equal(lab, np.fromfile(f32 / "000.labels", np.int32))
    assert open(os.path.join(str(tmp_path), "out_u8", "000.labels"), "rb").read() == open(f32 / "000.labels", "rb").read()


def test_writer_error_returns(tmp_path):
    from resnet_amd import binding as B
    lib = B.load()
    d = str(tmp_path).encode()
    assert lib.mi_build_shard_u8(str(tmp_path / "missing.csv").encode(), d, d, 0, 256) == -1
    csv = tmp_path / "000_images.csv"
    csv.write_text("005,0000,00,00\n")
    assert lib.mi_build_shard_u8(str(csv).encode(), d, d, 0, 256) == -2  # no class file
    (tmp_path / "00000005.buffer").write_bytes(b"\x01" * 1000)
    assert lib.mi_build_shard_u8(str(csv).encode(), d, d, 0, 256) == -4  # class file shorter than the image


def test_decode_model_reproduces_the_reference_fixture(tmp_path):
    """augref.decode of the uint8 shard with its FIXED crops = the fp32 shard the REFERENCE binary wrote from the same inputs"""
    img, lab, crops, _ = build_u8(str(tmp_path))
    pl = augref.plan(augref.FIXED, 0, 0, 0, 0, len(ROWS), DIM_IN, DIM_OUT, crops)
    out = augref.decode(img, pl, DIM_OUT).ravel()
    gold = np.load(os.path.join(GOLD, "shard_ref_golden.npz"))
    assert np.array_equal(lab, gold["labels"])
    assert out.size == int(gold["n_floats"])
    assert np.array_equal(out[:64].view(np.uint32), gold["head"].view(np.uint32))
    assert np.array_equal(out[-64:].view(np.uint32), gold["tail"].view(np.uint32))
    assert hashlib.sha256(out.tobytes()).hexdigest() == str(gold["sha256"])


def test_plan_matches_the_model():
    n, dim_in, dim_out = 64, 256, 224
    rng = np.random.RandomState(5)
    fixed = rng.randint(0, dim_in - dim_out + 1, size=(n, 2)).astype(np.int32)
    rc, got = c_plan(augref.FIXED, 1, 99, 3, 12345, n, dim_in, dim_out, fixed)
    assert rc == 0 and np.array_equal(got, augref.plan(augref.FIXED, 1, 99, 3, 12345, n, dim_in, dim_out, fixed))
    assert np.array_equal(got[:, :2], fixed) and not got[:, 2].any()
    rc, got = c_plan(augref.CENTER, 1, 99, 3, 12345, n, dim_in, dim_out)
    assert rc == 0 and np.array_equal(got, augref.plan(augref.CENTER, 1, 99, 3, 12345, n, dim_in, dim_out))
    assert np.all(got[:, :2] == 16) and not got[:, 2].any()
    for seed in (0, 7, 1234, 2 ** 63 + 5):
        for epoch in (0, 1, 5):
            for first in (0, 4096, 2 ** 31 + 17, 3 * 2 ** 33):  # a global index beyond 2^31
                for flip in (0, 1):
                    for di, do in ((256, 224), (40, 32), (37, 30), (32, 32)):
                        rc, got = c_plan(augref.RANDOM, flip, seed, epoch, first, n, di, do)
                        ref = augref.plan(augref.RANDOM, flip, seed, epoch, first, n, di, do)
                        assert rc == 0 and np.array_equal(got, ref), (seed, epoch, first, flip, di, do)
                        assert got[:, :2].min() >= 0 and got[:, :2].max() <= di - do
                        assert flip or not got[:, 2].any()
    # the draw of an image depends on its global index only, not on where the batch starts
    _, a = c_plan(augref.RANDOM, 1, 7, 2, 100, 32, 256, 224)
    _, b = c_plan(augref.RANDOM, 1, 7, 2, 116, 16, 256, 224)
    assert np.array_equal(a[16:], b)


def test_plan_error_returns():
    from resnet_amd import binding as B
    lib = B.load()
    assert c_plan(augref.FIXED, 0, 0, 0, 0, 4, 256, 224, None)[0] == -1  # FIXED without crops
    assert c_plan(augref.FIXED, 0, 0, 0, 0, 1, 256, 224, np.array([[33, 0]]))[0] == -1  # crop outside the image
    assert c_plan(3, 0, 0, 0, 0, 4, 256, 224)[0] == -1
    assert c_plan(augref.CENTER, 0, 0, 0, 0, 4, 224, 256)[0] == -1
    assert lib.mi_last_error().decode() != ""
    lib.mi_clear_error()


def test_random_plan_statistics():
    """R = 32, 4096 images per epoch: every offset occurs, about half the images are flipped, epochs differ.  The bounds hold for the
    model alone (an offset value is missed by 4096 uniform draws over 33 values with probability ~ 33 (32/33)^4096 < 1e-50; the flip
    share of 4096 fair coins has a standard deviation of 0.0078, so 0.46 .. 0.54 is five of them)"""
    n, dim_in, dim_out = 4096, 256, 224
    for seed in (1234, 7, 99):
        plans = []
        for epoch in range(3):
            rc, p = c_plan(augref.RANDOM, 1, seed, epoch, 0, n, dim_in, dim_out)
            assert rc == 0
            assert set(p[:, 0]) == set(range(33)) and set(p[:, 1]) == set(range(33))
            assert 0.46 <= p[:, 2].mean() <= 0.54
            plans.append(p)
        assert not np.array_equal(plans[0], plans[1]) and not np.array_equal(plans[1], plans[2])
        assert np.mean(plans[0][:, 0] == plans[1][:, 0]) < 0.1  # chance level is 1/33
