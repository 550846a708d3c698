"""The antialiased resize off the device (include/resnet_mi.h, "antialiased resize"): the numpy model (tests/aaref.py) against Pillow
itself and against the fixture Pillow wrote (tests/golden/aa_golden.npz), and the library's tap table mi_aa_coeffs -- compiled from the
text the kernel compiles -- against the model's.  CPU only; everything is compared bit for bit."""
import importlib.util
import os
import re

import numpy as np
import pytest

import aaref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "aa_golden.npz")


def model_resize(img, box, V):
    r0, c0, h, w = (int(v) for v in box)
    return aaref.resize(img[r0:r0 + h, c0:c0 + w, :], V)


def test_model_equals_pillow_on_a_seeded_sweep():
    pytest.importorskip("PIL")
    spec = importlib.util.spec_from_file_location("make_aa_golden", os.path.join(HERE, "golden", "make_aa_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    most_taps, shapes = 0, set()
    for k, (img, box, V) in enumerate(mk.cases(300, np.random.RandomState(7), 96, 64)):
        want, got = mk.pillow_resize(img, box, V), model_resize(img, box, V)
        assert got.shape == want.shape and np.array_equal(got, want), (k, img.shape, box, V, np.argwhere(got != want)[:1])
        most_taps = max(most_taps, max(len(aaref.taps(box[2], V, o)[1]) for o in range(V)))
        shapes.add((box[2] > V, box[3] > V))
    assert most_taps >= 40 and len(shapes) == 4  # strong downscales, and up / down on either axis in every combination
    # the validation resize: 256 -> 232, the centre 224^2 of it
    img = np.random.RandomState(8).randint(0, 256, size=(256, 256, 3), dtype=np.uint8)
    want, got = mk.pillow_resize(img, (0, 0, 256, 256), 232), model_resize(img, (0, 0, 256, 256), 232)
    assert np.array_equal(got, want) and np.array_equal(got[4:228, 4:228], want[4:228, 4:228])


def test_model_equals_the_fixture_pillow_wrote():
    g = np.load(GOLD)
    n = int(g["n"])
    assert n >= 36 and os.path.getsize(GOLD) < 200 * 1024
    kinds = set()
    for k in range(n):
        img, box, want = g["img%02d" % k], g["box%02d" % k], g["res%02d" % k]
        got = model_resize(img, box, want.shape[0])
        assert got.shape == want.shape and np.array_equal(got, want), (k, img.shape, box, want.shape)
        kinds.add((box[2] > want.shape[0], box[3] > want.shape[0]))
    assert len(kinds) == 4


def test_skipped_pass_is_the_table_that_hands_bytes_through():
    """in == V: Pillow skips the pass; the table K = (2^22, 0) the kernel runs instead gives the same bytes"""
    for n in (1, 2, 7, 224):
        m = aaref.table(n, n)
        assert np.array_equal(m, np.eye(n, dtype=np.int64) << 22)


def c_taps(lib, length, V, o, cap):
    K = np.full(cap + 2, -77, np.int32)
    xmin = np.array([-5], np.int32)
    n = lib.mi_aa_coeffs(length, V, o, xmin.ctypes.data, K.ctypes.data, cap)
    return n, int(xmin[0]), K


GRID = [(i, v) for i in (1, 2, 7, 8, 33, 96, 256) for v in (1, 4, 7, 24, 176, 224, 232)]
LONG = [(16384, 1), (16384, 7), (16384, 224), (16384, 16383), (1, 16384), (224, 16384), (16383, 16384)]


@pytest.mark.parametrize("length,V", GRID + LONG)
def test_mi_aa_coeffs_is_the_models_table(length, V):
    from resnet_amd import binding as B
    lib = B.load()
    cap = aaref.ksize(length, V)
    outs = range(V) if V <= 256 else sorted(set(np.random.RandomState(V).randint(0, V, 200).tolist() + [0, 1, V // 2, V - 2, V - 1]))
    for o in outs:
        xmin, K = aaref.taps(length, V, o)
        n, cx, cK = c_taps(lib, length, V, o, cap)
        assert 1 <= n <= cap and (n, cx) == (len(K), xmin), (o, n, cx, len(K), xmin)
        assert np.array_equal(cK[:n], K), (o, np.argwhere(cK[:n] != K)[:1])
        assert np.all(cK[n:] == -77)  # nothing behind the taps is written
        assert abs(int(K.sum()) - (1 << 22)) <= n and 255 * int(K.sum()) + (1 << 21) < 2 ** 31
        # the kernel's two min(sum >> 22, 255) never clamp: 256 would take a coefficient sum 8225 units high (no mutant is planted there)
        assert np.all(K >= 0) and (255 * int(K.sum()) + (1 << 21)) >> 22 == 255


# ---------------------------------------------------------------- the planted faults of tests/mutants.py, restated (no GPU)
# Every aa_* mutant is restated here in a numpy copy of the kernel's own structure -- the column table by window column (flip folded in),
# the column pass rounded to bytes, one row table PER WORKGROUP of R = aaref.launch_rows rows, the row pass by work item (quads, then the
# scalar tail), aa_value, the element-wise store -- and held, as a condition on the inputs the GPU tests build (same sources, seeds and
# box sets: they are imported from tests/test_gpu_input_aa.py), to change at least one element of every case that is named as its killer.
AA_THREADS = 256
FAULTS = ("aa_col_truncates", "aa_row_truncates", "aa_tail_truncates", "aa_value_r_plane_b_mean", "aa_scalar_store_lane3",
          "aa_ctab_first_coeff_low", "aa_rtab_last_coeff_high", "aa_col_blue_first_tap_zero", "aa_row_second_turn_plus_one",
          "aa_ctab_past_256_first_tap_zero", "aa_stage_pieces_past_64_zero", "aa_rtab_row9_first_tap_zero")


def kernel_model(src, boxes, D, virt=None, win=(0, 0), fault=None, aligned=True):
    """resample_aa_u8_kernel step by step, with one of FAULTS planted (None: aaref.resample's bits).  aligned: out on a 16-byte boundary"""
    import augref
    import rrcref
    n, dim_in = src.shape[0], src.shape[1]
    virt = D if virt is None else virt
    wr, wc = (win, win) if np.isscalar(win) else win
    R, Q, half = aaref.launch_rows(dim_in, D, virt), D // 4, 1 << (aaref.BITS - 1)
    vec = D % 4 == 0 and aligned
    out = np.empty((n, 3, D, D), np.float32)

    def to_byte(acc):  # min(s >> 22, 255) stored as an unsigned char
        return np.minimum(acc >> aaref.BITS, 255) & 255

    for im in range(n):
        r0, c0, h, w, fl = rrcref.clamp_box(boxes[im], dim_in)
        box = src[im, r0:r0 + h, c0:c0 + w, :].astype(np.int64)
        if fault == "aa_stage_pieces_past_64_zero":  # a row's 16-byte pieces are counted from its span's start rounded down to 16
            xa = aaref.taps(w, virt, wc)[0]
            g = (((im * dim_in + r0 + np.arange(h)) * dim_in + c0 + xa) * 3)[:, None]
            gone = (g & 15) + np.arange((w - xa) * 3)[None, :] >= 64 * 16
            box[:, xa:, :] = np.where(gone, 0, box[:, xa:, :].reshape(h, -1)).reshape(h, w - xa, 3)
        ctab = np.zeros((D, w), np.int64)
        first = np.zeros((D, w), np.int64)  # the first coefficient of every entry alone
        for i in range(D):
            lo, K = aaref.taps(w, virt, wc + (D - 1 - i if fl else i))
            K = K.copy()
            if fault == "aa_ctab_first_coeff_low":
                K[0] -= len(K) > 1
            if fault == "aa_ctab_past_256_first_tap_zero" and i >= AA_THREADS:
                K[0] = 0
            ctab[i, lo:lo + len(K)] = K
            first[i, lo] = K[0]
        acc = np.einsum("ij,rjc->ric", ctab, box) + (0 if fault == "aa_col_truncates" else half)
        if fault == "aa_col_blue_first_tap_zero":
            acc[:, :, 0] -= np.einsum("ij,rj->ri", first, box[:, :, 0])
        mid = to_byte(acc)  # (h, D, 3)
        byte = np.zeros((D, D, 3), np.int64)
        for h0 in range(0, D, R):
            for i in range(min(R, D - h0)):
                lo, K = aaref.taps(h, virt, wr + h0 + i)
                K = K.copy()
                if fault == "aa_rtab_last_coeff_high":
                    K[-1] += len(K) > 1
                if fault == "aa_rtab_row9_first_tap_zero" and i == 9:
                    K[0] = 0
                s = np.tensordot(K, mid[lo:lo + len(K)], axes=(0, 0))  # (D, 3)
                start = np.full((D, 1), half, np.int64)
                if fault == "aa_row_truncates":
                    start[:4 * Q] = 0
                if fault == "aa_tail_truncates":
                    start[4 * Q:] = 0
                b = np.minimum((s + start) >> aaref.BITS, 255)
                if fault == "aa_row_second_turn_plus_one":
                    item = i * Q + np.arange(D) // 4  # the work item of a quad's columns
                    b[:4 * Q] += (item[:4 * Q] >= AA_THREADS)[:, None]
                byte[h0 + i] = b
        for d in range(3):
            p = 2 - d
            mean = augref.MEAN_OF_SRC[0 if fault == "aa_value_r_plane_b_mean" and p == 2 else p]
            v = (byte[:, :, p].astype(np.float32).astype(np.float64) - mean).astype(np.float32)
            if fault == "aa_scalar_store_lane3" and not vec:
                v[:, 3:4 * Q:4] += np.float32(0.0625)
            out[im, d] = v
    return out


def _gpu_cases():
    import test_gpu_input_aa as G
    return G


def _case_id(case):
    return "-".join("win%d" % _gpu_cases().CASES.index(case) if isinstance(v, tuple) else str(v) for v in case)


def _killer_inputs(node):
    """the (name of the input set, src, boxes, case, aligned) a killer node id of tests/mutants.py runs"""
    G = _gpu_cases()
    if node == "tests/test_gpu_input_aa.py::test_refuses_an_image_too_wide_for_lds":
        D, dim_in, img, whole = G.lds_limit_inputs()
        return [("whole, flipped", img, whole, (dim_in - 1, D, D, 0), True)]
    test, ident = re.fullmatch(r"tests/test_gpu_input_aa\.py::(\w+)\[(.+)\]", node).groups()
    case = next(c for c in G.CASES if _case_id(c) == ident)
    dim_in, virt = case[0], case[1]
    if test == "test_sweep":
        sets = G.box_sets(dim_in, np.random.RandomState(dim_in * 100 + virt))
        return [(k, G.source(dim_in), np.array(b, np.int32), case, True) for k, b in sets.items()]
    assert test == "test_into_an_output_one_float_off_alignment"
    b = G.box_sets(dim_in, np.random.RandomState(3))["whole+corner"]
    return [("whole+corner", G.source(dim_in), np.array(b, np.int32), case, False)]


_TRUE = {}


def _differing(fault, node):
    """elements per input set of a killer in which the faulted model differs from aaref.resample"""
    counts = {}
    for name, src, boxes, (dim_in, virt, D, win), aligned in _killer_inputs(node):
        key = (node, name)
        if key not in _TRUE:
            _TRUE[key] = aaref.resample(src, boxes, D, virt, win)
        bad = kernel_model(src, boxes, D, virt, win, fault, aligned).view(np.uint32) != _TRUE[key].view(np.uint32)
        counts[name] = bad.reshape(len(boxes), -1).sum(axis=1)
    return counts


def test_new_cases_are_on_their_branches():
    _gpu_cases().test_new_cases_are_on_their_branches()


def test_every_aa_mutant_is_restated():
    import mutants
    assert sorted(m["name"] for m in mutants.MUTANTS if m["name"].startswith("aa_")) == sorted(FAULTS)
    assert all(m["file"] == "kernels_input.hip" for m in mutants.MUTANTS if m["name"].startswith("aa_"))


def test_kernel_model_without_a_fault_is_the_model():
    G = _gpu_cases()
    for case in G.CASES:
        for name, src, boxes, (dim_in, virt, D, win), _ in _killer_inputs("tests/test_gpu_input_aa.py::test_sweep[%s]" % _case_id(case)):
            a, b = kernel_model(src, boxes, D, virt, win), aaref.resample(src, boxes, D, virt, win)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (case, name)


ROW9 = "aa_rtab_row9_first_tap_zero"


@pytest.mark.parametrize("fault", FAULTS)
def test_every_killer_separates_its_mutant(fault):
    """each killer's own inputs change under the fault (the one exception is the second killer of the row-9 entry: R = 9 there, and the
    condition is that NOTHING changes)"""
    import mutants
    m = mutants.by_name(fault)
    for node in m["killers"]:
        counts = _differing(fault, node)
        total = int(sum(c.sum() for c in counts.values()))
        print("%s on %s: %d elements differ %s" % (fault, node.split("::")[1], total, {k: v.tolist() for k, v in counts.items()}))
        if fault == ROW9 and "[200-24-24-0]" in node:
            assert total == 0, counts
        else:
            assert total > 0, "%s cannot kill %s: the fault changes nothing on its inputs" % (node, fault)
    if fault == ROW9:  # R = 16: window row 9 and no other, in every image
        G = _gpu_cases()
        src, boxes = G.source(16), np.array(G.box_sets(16, np.random.RandomState(3))["whole+corner"], np.int32)
        bad = kernel_model(src, boxes, 24, 24, 0, fault).view(np.uint32) != aaref.resample(src, boxes, 24, 24, 0).view(np.uint32)
        assert all(b.any(axis=(0, 2)).tolist() == [r == 9 for r in range(24)] for b in bad)


TIE_PRONE = [(16, 24, 24, 0), (64, 58, 52, 3)]


@pytest.mark.parametrize("fault", ["aa_ctab_first_coeff_low", "aa_rtab_last_coeff_high"])
def test_one_unit_coefficient_faults_need_a_tie_prone_ratio(fault):
    """one unit of 2^-22 in one coefficient of ONE pass (the column table alone, the row table alone) moves an output only where a sum
    lies within one byte value of a rounding boundary.  The condition: the mutant's killers are tie-prone ratios, and each of them changes
    in EACH of the three whole+corner images; whole images at ratios with an odd small denominator (9 -> 4, 33 -> 7) change
    nowhere"""
    import mutants
    killers = mutants.by_name(fault)["killers"]
    ids = [re.search(r"\[(.+)\]", k).group(1) for k in killers]
    assert all(i in [_case_id(c) for c in TIE_PRONE] for i in ids), ids
    per_image = []
    for k in killers:
        c = _differing(fault, k)["whole+corner"]
        print("%s on %s, whole+corner: %s elements differ per image" % (fault, k.split("::")[1], c.tolist()))
        per_image.append(c)
    assert all((c >= 1).all() for c in per_image), per_image
    for case in ((9, 4, 4, 0), (33, 7, 7, 0)):
        blind = _differing(fault, "tests/test_gpu_input_aa.py::test_sweep[%s]" % _case_id(case))["whole+corner"]
        assert blind[:2].sum() == 0, (case, blind)  # the two whole-image boxes: the case's own ratio


@pytest.mark.parametrize("fault,first", [("aa_row_second_turn_plus_one", (100, 68, 68, 0)), ("aa_ctab_past_256_first_tap_zero", (300, 260, 260, 0))])
def test_later_turn_faults_survive_every_older_case(fault, first):
    """the survivor prediction: on every case the module had before, in every box set and off alignment, the faulted model IS the model;
    on the case added for the turn it is not"""
    G = _gpu_cases()
    nodes = ["tests/test_gpu_input_aa.py::test_sweep[%s]" % _case_id(c) for c in G.OLD_CASES]
    nodes += ["tests/test_gpu_input_aa.py::test_into_an_output_one_float_off_alignment[%s]" % i for i in ("32-8-8-0", "64-58-52-3")]
    nodes.append("tests/test_gpu_input_aa.py::test_refuses_an_image_too_wide_for_lds")
    for node in nodes:
        assert sum(int(c.sum()) for c in _differing(fault, node).values()) == 0, node
    # the other tests of the module launch dim_out <= 32 as well (the decode and upscale comparisons, the loader, the evaluation)
    counts = _differing(fault, "tests/test_gpu_input_aa.py::test_sweep[%s]" % _case_id(first))
    print("%s on %s: %s" % (fault, first, {k: v.tolist() for k, v in counts.items()}))
    assert sum(int(c.sum()) for c in counts.values()) > 0, counts


def test_mi_aa_coeffs_honours_cap_and_refuses_nonsense():
    from resnet_amd import binding as B
    lib = B.load()
    xmin, K = aaref.taps(96, 7, 3)
    n, cx, cK = c_taps(lib, 96, 7, 3, 5)
    assert n == len(K) > 5 and cx == xmin and np.array_equal(cK[:5], K[:5]) and np.all(cK[5:] == -77)
    for bad in ((0, 4, 0), (4, 0, 0), (4, 4, 4), (4, 4, -1)):
        assert c_taps(lib, *bad, 8)[0] == -1
        assert "mi_aa_coeffs" in lib.mi_last_error().decode()
        lib.mi_clear_error()
