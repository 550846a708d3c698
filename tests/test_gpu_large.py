"""Every kernel family on tensors past 2 GiB and 4 GiB: the result is right to the suite's own bounds, or the call refuses, names the size
limit and launches nothing.  A wrong result with return code 0 is what these tests exist to catch.

The hot kernels address memory as a wave-uniform 64-bit base plus a 32-bit per-lane byte offset, or with 32-bit element indices; the limits
that follow are DESIGN.md's "Size limits" table and tests/test_large_plan.py pins where the planner puts them.  Here the kernels run at
those sizes.  Each case is one launch of one operator on operands filled on the device, and slab copies (tests/largeref.py): whole images
0, N - 1, the image that holds the element at byte offset 2^31 (2^32) with its neighbours, two seeded ones -- every channel of them,
against convref's / ewref's float64 references and per-element bounds, unchanged.  Reductions over the batch (weight gradients, BN
statistics, BN' sums) take the sparse form: zeros everywhere but in the slab images.  N is the smallest batch that leaves three whole
images past the boundary (672 at 802816 floats per image; the 200704- and 401408-element images take 2680, bf16 802816 takes 1344), or
the planner's own answer for the top of a route's range and the first batch past it.  Every case asserts, through mi_debug_trace_names,
which kernel ran.

Peak device bytes of a case's own tensors are listed at the end of the module with its seconds and its worst distance from the bound (the
operators' workspaces, at most a few hundred MB, come on top).  Measured: 2.6 - 8.6 GB for the convolutions, up to 15.1 GB for the bf16
element-wise cases (bf16 operands are filled as fp32 in scratch), 17.2 and 21.5 GB for BN and pooling at 2^31 elements, 34.4 GB for the
2^32-element refusals (allocated whole, so that a missing guard could not write outside them).  An allocation that fails is a failure.

Sections: (a) fp32 past 2^31 bytes on the default routes, (b) bf16 past 2^31 bytes, (c) the top of each accepted range, (d) the first
batch past the fp32 implicit GEMM's limit and three images further (the direct kernel's former 32-bit row offsets went wrong from image
5350 on: tests/test_large_plan.py restates them), (e) the element-wise family past 2^31 bytes, (f) BN and pooling at 2^31 and 2^32
elements.
"""
import ctypes
import time

import numpy as np
import pytest

import convref as R
import ewref as E
import largeref as G
import lossref
import optim_ref

pytestmark = pytest.mark.gpu

F32, BF16 = G.F32, G.BF16
EPS = E.EPS
REPORT = []   # (case, seconds, peak device bytes, worst distance, unit)


@pytest.fixture(scope="module")
def L(ops):
    R.set_threads(16)
    lib = ops.L
    lib.mi_clear_error()
    yield lib
    print("\ncase | seconds | peak device bytes | worst distance")
    for row in REPORT:
        print("  %-58s %6.1f  %12d  %.3g %s" % row)


class Case:
    """one case: its arena, its clock, and the line it leaves in REPORT"""

    def __init__(self, L, name):
        self.L, self.name, self.worst, self.unit = L, name, 0.0, ""

    def __enter__(self):
        self.t0 = time.time()
        self.L.mi_clear_error()
        self.a = G.Arena(self.L)
        return self

    def __exit__(self, et, ev, tb):
        self.a.close()
        if et is None:
            REPORT.append((self.name, time.time() - self.t0, self.a.peak, self.worst, self.unit))
        return False

    def run(self, fn, *args):
        """the operator call, with the launch ring cleared in front of it"""
        self.L.mi_debug_trace_clear()
        return getattr(self.L, fn)(*args)

    def ok(self, rc, what):
        assert rc >= 0, "%s failed (%d): %s" % (what, rc, self.L.mi_last_error().decode())

    def check(self, got, ref, A, bf, what):
        w, bad = (R.dist_bf16 if bf else R.dist_f32)(got, ref, A)
        assert bad == 0, "%s %s: %d elements out of bounds (worst %.3g %s)" % (self.name, what, bad, w, "bf16 ulp" if bf else "x 2^-24 A")
        self.worst, self.unit = max(self.worst, w), "bf16 ulp" if bf else "x 2^-24 A"
        return w

    def exact(self, got, want, what):
        got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
        assert got.shape == want.shape and got.dtype == want.dtype, what
        bits = np.uint32 if got.dtype.itemsize == 4 else np.uint16
        assert np.array_equal(got.view(bits), want.view(bits)), "%s %s: %d of %d elements differ" % (self.name, what, np.count_nonzero(got != want), got.size)
        self.unit = self.unit or "(bit for bit)"


def images_of(N, sizes, item, seed, need_past):
    """the slab images of a case: largeref.boundary_images over every tensor of the case (need_past holds for the largest)"""
    big = max(sizes)
    s = set()
    for e in sizes:
        s.update(G.boundary_images(N, e, item, seed, need_past if e == big else 0))
    return sorted(s)


def weights(K, C, k, seed, bf):
    w = (np.random.default_rng(seed).standard_normal((K, C, k, k), dtype=np.float32) * np.float32((2.0 / (k * k * (C + K))) ** 0.5))
    return R.bf16_round32(w) if bf else w


def slab_data(S, shape, seed, bf):
    """real data for the slab images of a sparse operand"""
    a = np.random.default_rng(seed).uniform(-1.0, 1.0, (len(S),) + shape).astype(np.float32)
    return R.bf16_round32(a) if bf else a


# ---------------------------------------------------------------------------------------------------------------------------
# convolutions
CONV_FN = {
    ("f32", "default"): ("mi_op_conv_fwd", "mi_op_conv_dgrad", "mi_op_conv_wgrad"),
    ("bf16", "default"): ("mi_op_conv_fwd_bf16", "mi_op_conv_dgrad_bf16", "mi_op_conv_wgrad_bf16"),
    ("bf16", "cl"): ("mi_op_conv_fwd_bf16_cl", "mi_op_conv_dgrad_bf16_cl", "mi_op_conv_wgrad_bf16_cl"),
    ("bf16", "cl2"): (None, None, "mi_op_conv_wgrad_bf16_cl2"),
}
OPI = {"fwd": 0, "dgrad": 1, "wgrad": 2}


def conv_call(c, dtn, route, op, ptrs, N, shape):
    """ptrs in the operator's order: fwd (x, w, y), dgrad (w, dy, dx), wgrad (x, dy, dw)"""
    C, H, K, k, s = shape
    fn = CONV_FN[(dtn, route)][OPI[op]]
    tail = (N, C, H, K, s) if route in ("cl", "cl2") else (N, C, H, K, k, s)
    if op == "dgrad":
        tail += (0,)
    return c.run(fn, *(ptrs + tail))


def conv_case(L, dtn, route, op, shape, N, names, need_past=3, contract=False, tag=""):
    """one convolution operator at batch N on its slab images; contract: a refusal that names the limit also passes (case (d))"""
    C, H, K, k, s = shape
    bf = dtn == "bf16"
    dt, item = (BF16, 2) if bf else (F32, 4)
    Ho = H // s
    Ein, Eout = C * H * H, K * Ho * Ho
    seed = (C * 31 + K * 7 + H + k + s + OPI[op]) % 1000
    S = images_of(N, (Ein, Eout), item, seed, need_past)
    w = weights(K, C, k, seed + 1, bf)
    with Case(L, "%s%s %s %s C%d H%d K%d k%d s%d N%d" % (tag, dtn, route, op, C, H, K, k, s, N)) as c:
        a = c.a
        wd = a.upload(w)
        if op == "fwd":
            x, y = a.new_filled(N * Ein, 1000 + seed, -1.0, 1.0, dt), a.new_poisoned(N * Eout, dt)
            rc = conv_call(c, dtn, route, op, (x, wd, y), N, shape)
        elif op == "dgrad":
            dy, dx = a.new_filled(N * Eout, 2000 + seed, -1.0, 1.0, dt), a.new_poisoned(N * Ein, dt)
            rc = conv_call(c, dtn, route, op, (wd, dy, dx), N, shape)
        else:
            xs, dys = slab_data(S, (C, H, H), seed + 2, bf), slab_data(S, (K, Ho, Ho), seed + 3, bf)
            x, dy = a.new_zero(N * Ein, dt), a.new_zero(N * Eout, dt)
            a.write_images(x, S, Ein, xs, dt)
            a.write_images(dy, S, Eout, dys, dt)
            dw = a.new_poisoned(K * C * k * k)
            rc = conv_call(c, dtn, route, op, (x, dy, dw), N, shape)
        if contract and rc != 0:
            G.assert_refused(L, rc, c.name)
            c.unit = "(refused)"
            return
        c.ok(rc, c.name)
        assert rc == 0
        G.assert_launched(L, names, c.name)
        if op == "fwd":
            xs = G.regen_images(1000 + seed, -1.0, 1.0, S, Ein, dt).reshape(len(S), C, H, H)
            got = a.read_images(y, S, Eout, dt).reshape(len(S), K, Ho, Ho)
            c.check(got, R.fwd64(xs, w, s), R.fwd64(np.abs(xs), np.abs(w), s), bf, "images %s" % (S,))
        elif op == "dgrad":
            dys = G.regen_images(2000 + seed, -1.0, 1.0, S, Eout, dt).reshape(len(S), K, Ho, Ho)
            got = a.read_images(dx, S, Ein, dt).reshape(len(S), C, H, H)
            c.check(got, R.dgrad64(w, dys, H, s), R.dgrad64(np.abs(w), np.abs(dys), H, s), bf, "images %s" % (S,))
        else:
            got = a.download(dw, K * C * k * k).reshape(K, C, k, k)
            c.check(got, R.wgrad64(xs, dys, k, s), R.wgrad64(np.abs(xs), np.abs(dys), k, s), False, "the sum over images %s" % (S,))


def ig(op, k, s):
    return "igemm_kernel<%s,k%d,s%d" % (op, k, s)


def bg(op, k, s):
    return "bgemm_kernel<%s,k%d,s%d" % (op, k, s)


A_CONV = [   # (a) fp32 past 2^31 bytes on the default routes: (op, shape, N, launch names)
    ("fwd", (256, 56, 64, 1, 1), 672, [ig("fwd", 1, 1)]), ("dgrad", (256, 56, 64, 1, 1), 672, [ig("dgrad", 1, 1)]),
    ("fwd", (64, 56, 256, 1, 1), 672, [ig("fwd", 1, 1)]), ("dgrad", (64, 56, 256, 1, 1), 672, [ig("dgrad", 1, 1)]),
    ("fwd", (64, 56, 64, 3, 1), 2680, [ig("fwd", 3, 1)]), ("dgrad", (64, 56, 64, 3, 1), 2680, [ig("dgrad", 3, 1)]),
    ("wgrad", (64, 56, 64, 3, 1), 2680, [ig("wgrad", 3, 1)]),
    ("fwd", (256, 56, 512, 3, 2), 672, [ig("fwd", 3, 2)]), ("dgrad", (256, 56, 512, 3, 2), 672, [ig("dgrad", 3, 2)]),
    ("wgrad", (256, 56, 512, 3, 2), 672, [ig("wgrad", 3, 2)]),
    ("wgrad", (256, 56, 64, 1, 1), 672, [ig("wgrad", 1, 1)]), ("wgrad", (64, 56, 256, 1, 1), 672, [ig("wgrad", 1, 1)]),
]


@pytest.mark.parametrize("case", A_CONV, ids=["%s_C%d_H%d_K%d_k%d_s%d" % ((c[0],) + c[1]) for c in A_CONV])
def test_a_fp32_convolution_past_2_gib(L, case):
    op, shape, N, names = case
    conv_case(L, "f32", "default", op, shape, N, names)


def _pw_wgrad(L, N, shape):
    C, H, K, k, s = shape
    return ["pw_wgrad_kernel"] if L.mi_bf16_pw_wgrad_supported(N, C, H, K) else [bg("wgrad", 1, 1)]


B_CONV = [   # (b) bf16 past 2^31 bytes (2^30 elements): (route, op, shape, N, launch names; None: the 1x1 weight gradient's launch-time choice)
    ("default", "fwd", (256, 56, 64, 1, 1), 1344, [bg("fwd", 1, 1)]), ("default", "dgrad", (256, 56, 64, 1, 1), 1344, [bg("dgrad", 1, 1)]),
    ("default", "wgrad", (256, 56, 64, 1, 1), 1344, None),
    ("default", "fwd", (64, 56, 256, 1, 1), 1344, [bg("fwd", 1, 1)]), ("default", "dgrad", (64, 56, 256, 1, 1), 1344, [bg("dgrad", 1, 1)]),
    ("default", "wgrad", (64, 56, 256, 1, 1), 1344, None),
    ("default", "wgrad", (256, 56, 128, 1, 1), 1344, None),   # (both channel counts a multiple of 128: the LDS-DMA kernel, pw_wgrad_kernel)
    ("cl", "fwd", (128, 56, 128, 3, 1), 2680, ["cl_relayout", "cl_conv_kernel<taps9"]),
    ("cl", "dgrad", (128, 56, 128, 3, 1), 2680, ["cl_relayout", "cl_conv_kernel<taps9"]),
    ("cl", "wgrad", (128, 56, 128, 3, 1), 2680, ["cl_relayout", "cl_wgrad_kernel"]),
    ("cl", "fwd", (128, 56, 256, 3, 2), 2680, ["cl_relayout", "cl_conv_kernel<taps9"]),
    ("cl", "dgrad", (128, 56, 256, 3, 2), 2680, ["cl_relayout64_kernel", "cl_dgrad2_kernel"]),
    ("cl2", "wgrad", (128, 56, 256, 3, 2), 2680, ["cl_relayout", "cl_wgrad2_kernel"]),
    ("default", "fwd", (128, 56, 256, 3, 2), 2680, ["bg_s2d_kernel", bg("fwd", 3, 2)]),
    ("default", "dgrad", (128, 56, 256, 3, 2), 2680, [bg("dgrad", 3, 2)]),
    ("default", "wgrad", (128, 56, 256, 3, 2), 2680, [bg("wgrad", 3, 2)]),
]


@pytest.mark.parametrize("case", B_CONV, ids=["%s_%s_C%d_H%d_K%d_k%d_s%d" % (c[:2] + c[2]) for c in B_CONV])
def test_b_bf16_convolution_past_2_gib(L, case):
    route, op, shape, N, names = case
    conv_case(L, "bf16", route, op, shape, N, names if names is not None else _pw_wgrad(L, N, shape))


def _last_accepted(accepts, lo=256, hi=1 << 24):
    assert accepts(lo) and not accepts(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if accepts(mid) else (lo, mid)
    return lo


def _igemm_takes(L, op, N, shape):
    out = (ctypes.c_int * 9)()
    L.mi_debug_conv_plan(op, N, *shape, out)
    return out[0] == 1


@pytest.mark.parametrize("op", ["fwd", "dgrad"])
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
def test_c_top_of_the_accepted_range(L, dtn, op):
    """1x1 256 -> 64 @56 at the largest N the planner accepts (fp32 1337, bf16 2674: the last byte offsets sit just under 2^32, with
    BG_BIAS added in the bf16 kernel): the margin of the guard"""
    shape = (256, 56, 64, 1, 1)
    if dtn == "f32":
        N = _last_accepted(lambda n: _igemm_takes(L, OPI[op], n, shape))
        names = [ig(op, 1, 1)]
    else:
        N = _last_accepted(lambda n: L.mi_bf16_conv_supported(OPI[op], n, *shape) == 1)
        names = [bg(op, 1, 1)]
    assert N == (1337 if dtn == "f32" else 2674)
    conv_case(L, dtn, "default", op, shape, N, names, need_past=0, tag="top ")


D_CONV = [((256, 56, 64, 1, 1), 0, ["gemm_mfma_kernel"]), ((64, 56, 64, 3, 1), 0, ["dconv_kernel<t3x3"]), ((64, 56, 64, 3, 1), 3, ["dconv_kernel<t3x3"])]


@pytest.mark.parametrize("op", ["fwd", "dgrad"])
@pytest.mark.parametrize("case", D_CONV, ids=["C%d_H%d_K%d_k%d_s%d_plus%d" % (c[0] + (c[1],)) for c in D_CONV])
def test_d_first_batch_past_the_fp32_limit(L, case, op):
    """the first N mi_igemm_supported declines (1338; 5350 for the 3x3), and for the 3x3 three images further (5353: from image 5350 on
    the direct kernel's row offsets no longer fit 32 bits).  The contract: right on the fallback route, or refused"""
    shape, plus, names = case
    N = _last_accepted(lambda n: _igemm_takes(L, OPI[op], n, shape)) + 1 + plus
    assert N == {1: 1338, 3: 5350}[shape[3]] + plus
    assert R.conv_plan(L, 0, "default", op, N, *shape) is None and R.layer_routes(L, 0, 0, N, *shape) == (0, 0, 0, 0)
    conv_case(L, "f32", "default", op, shape, N, names, need_past=0, contract=True, tag="past ")


# ---------------------------------------------------------------------------------------------------------------------------
# the stem
@pytest.mark.parametrize("op", ["fwd", "wgrad"])
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
def test_a_stem_past_2_gib(L, dtn, op):
    """3 -> 64 @224 at N = 672 on both matrix-core routes: the output (forward) and dY (weight gradient) cross 2^31 bytes"""
    N, H, bf = 672, 224, dtn == "bf16"
    Ho = H // 2
    Ein, Eout = 3 * H * H, 64 * Ho * Ho
    S = images_of(N, (Eout,), 4, 7, 3)
    w = weights(64, 3, 7, 42, bf)
    rnd = R.bf16_round32 if bf else (lambda v: v)
    with Case(L, "stem %s %s N%d" % (dtn, op, N)) as c:
        a = c.a
        wd = a.upload(w)
        if op == "fwd":
            x, y = a.new_filled(N * Ein, 41, -1.0, 1.0), a.new_poisoned(N * Eout)
            c.ok(c.run("mi_op_stem_fwd_bf16" if bf else "mi_op_stem_fwd_f32", x, wd, y, N, H), c.name)
            G.assert_launched(L, ["st_fwd_kernel<f32 out>" if bf else "st32_fwd_kernel"], c.name)
            xs = rnd(G.regen_images(41, -1.0, 1.0, S, Ein)).reshape(len(S), 3, H, H)
            got = a.read_images(y, S, Eout).reshape(len(S), 64, Ho, Ho)
            c.check(got, R.fwd64(xs, w, 2), R.fwd64(np.abs(xs), np.abs(w), 2), False, "images %s" % (S,))
        else:
            xs, dys = slab_data(S, (3, H, H), 43, bf), slab_data(S, (64, Ho, Ho), 44, bf)
            x, dy = a.new_zero(N * Ein), a.new_zero(N * Eout)
            a.write_images(x, S, Ein, xs)
            a.write_images(dy, S, Eout, dys)
            dw = a.new_poisoned(64 * 3 * 49)
            c.ok(c.run("mi_op_stem_wgrad_bf16" if bf else "mi_op_stem_wgrad_f32", x, wd, dy, dw, N, H), c.name)
            G.assert_launched(L, ["st_wgrad_kernel<f32 dy>" if bf else "st32_wgrad_kernel"], c.name)
            got = a.download(dw, 64 * 3 * 49).reshape(64, 3, 7, 7)
            c.check(got, R.wgrad64(xs, dys, 7, 2), R.wgrad64(np.abs(xs), np.abs(dys), 7, 2), False, "the sum over images %s" % (S,))


# ---------------------------------------------------------------------------------------------------------------------------
# convolution + BN pairs
def _bn_vectors(Cn, seed):
    rng = np.random.default_rng(seed)
    gamma = (1 + 0.3 * np.clip(rng.standard_normal(Cn), -2.5, 2.5)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(Cn)).astype(np.float32)
    return gamma, beta


def test_a_fused_conv_bn_forward_past_2_gib(L):
    """mi_op_conv_bn_fwd_t, fp32 64 -> 256 @56 at N = 672 (sparse input): the convolution on the slab images and exactly zero in another
    image, the statistics from the epilogue's partials against the float64 statistics of the exact convolution over all N images, the
    BN + ReLU output on the slab images"""
    N, (C, H, K, k, s) = 672, (64, 56, 256, 1, 1)
    Ein, Eout, P = C * H * H, K * H * H, H * H
    S = images_of(N, (Eout,), 4, 11, 3)
    w = weights(K, C, k, 12, False)
    gamma, beta = _bn_vectors(K, 13)
    xs = slab_data(S, (C, H, H), 14, False)
    with Case(L, "conv+bn fwd f32 C64 H56 K256 N672") as c:
        a = c.a
        x = a.new_zero(N * Ein)
        a.write_images(x, S, Ein, xs)
        conv, y = a.new_poisoned(N * Eout), a.new_poisoned(N * Eout)
        wd, gd, bd, md, vd = a.upload(w), a.upload(gamma), a.upload(beta), a.new_poisoned(K), a.new_poisoned(K)
        rc = c.run("mi_op_conv_bn_fwd_t", x, wd, conv, F32, gd, bd, md, vd, y, N, C, H, K, k, s, 1e-7, 1)
        c.ok(rc, c.name)
        assert rc > 0, "the statistics must come from the convolution's epilogue"
        G.assert_launched(L, [ig("fwd", 1, 1), "bn_parts_merge_kernel", "bn_apply_kernel<f32,f32,v4>"], c.name)
        ref, A = R.fwd64(xs, w, s), R.fwd64(np.abs(xs), np.abs(w), s)
        got = a.read_images(conv, S, Eout).reshape(len(S), K, H, H)
        c.check(got, ref, A, False, "convolution, images %s" % (S,))
        other = next(n for n in range(N - 2, 0, -1) if n not in S)
        assert not np.any(a.read(conv, other * Eout, Eout)), "image %d of a zero input is not zero" % other
        gm, gv = a.download(md, K), a.download(vd, K)
        bad, ws = G.stats_distance(gm, gv, G.sparse_stats_ref(ref, A, N * P))
        assert bad == 0, "statistics: %d values out of bounds, worst %.3g x 2^-24 (bound scale)" % (bad, ws)
        yr, yA = E.apply_ref(got, gamma, beta, gm, gv, 1e-7, True)
        c.check(a.read_images(y, S, Eout).reshape(got.shape), yr, yA, False, "BN + ReLU, images %s" % (S,))
        c.worst = max(c.worst, ws)


def test_a_fused_dgrad_bn_backward_past_2_gib(L):
    """mi_op_conv_dgrad_bn_bwd_f32, the 256 -> 64 @56 reduction at N = 672 (sparse dY): the gated dgrad on the slab images, dbeta and dgamma
    from the epilogue's partials against float64 sums of the stored gated gradient, BN' dx from those sums"""
    N, (C, H, K, k, s) = 672, (256, 56, 64, 1, 1)
    Ein, Eout, P = C * H * H, K * H * H, H * H
    S = images_of(N, (Ein,), 4, 21, 3)
    w = weights(K, C, k, 22, False)
    gamma, beta = _bn_vectors(C, 23)
    rng = np.random.default_rng(24)
    means, vars_ = rng.uniform(-0.2, 0.2, C).astype(np.float32), rng.uniform(0.2, 0.5, C).astype(np.float32)
    dys = slab_data(S, (K, H, H), 25, False)
    with Case(L, "dgrad+bn' f32 C256 H56 K64 N672") as c:
        a = c.a
        dy = a.new_zero(N * Eout)
        a.write_images(dy, S, Eout, dys)
        bn_x, mask = a.new_filled(N * Ein, 26, -1.0, 1.0), a.new_filled(N * Ein, 27, -1.0, 1.0)
        gated, bdx = a.new_poisoned(N * Ein), a.new_poisoned(N * Ein)
        wd, gd, bd, md, vd = a.upload(w), a.upload(gamma), a.upload(beta), a.upload(means), a.upload(vars_)
        dg, db = a.new_poisoned(C), a.new_poisoned(C)
        rc = c.run("mi_op_conv_dgrad_bn_bwd_f32", wd, dy, None, gated, N, C, H, K, k, s, bn_x, mask, gd, bd, md, vd, EPS, bdx, dg, db)
        c.ok(rc, c.name)
        assert rc > 0, "the dgrad on the implicit GEMM does the BN' reduction"
        G.assert_launched(L, [ig("dgrad", 1, 1), "bn_bwd_parts_merge_kernel", "bn_bwd_apply_kernel<f32,f32,v4>"], c.name)
        shp = (len(S), C, H, H)
        xb, mk = G.regen_images(26, -1.0, 1.0, S, Ein).reshape(shp), G.regen_images(27, -1.0, 1.0, S, Ein).reshape(shp)
        on = mk > 0
        ref, A = R.dgrad64(w, dys, H, s), R.dgrad64(np.abs(w), np.abs(dys), H, s)
        g = a.read_images(gated, S, Ein).reshape(shp)
        c.check(g, np.where(on, ref, 0.0), np.where(on, A, 0.0), False, "gated dgrad, images %s" % (S,))
        sums = R.bn_grad_sums(g, xb, means, vars_, EPS)     # every other image's gradient is exactly zero
        bad, ws = E.sums_violations(a.download(db, C), a.download(dg, C), sums)
        assert bad == 0, "dbeta / dgamma: %d values out of bounds (worst %.3g x 2^-24 sum|terms|)" % (bad, ws)
        xr, xA = E.dx_ref(g, xb, gamma, means, vars_, EPS, sums, N * P)
        c.check(a.read_images(bdx, S, Ein).reshape(shp), xr, xA, False, "BN' dx, images %s" % (S,))
        c.worst = max(c.worst, ws)


# ---------------------------------------------------------------------------------------------------------------------------
# (e) the element-wise family
EW_N, EW_C, EW_H = 2680, 64, 56


def _ew_geometry(dt, Cn=None, H=EW_H, N=EW_N):
    """fp32: 64 channels @56 at N = 2680; bf16: twice the elements (128 channels)"""
    Cn = Cn or (EW_C if dt == F32 else 2 * EW_C)
    Ei = Cn * H * H
    return N, Cn, H, Ei, images_of(N, (Ei,), G.ITEM[dt], Cn + H, 3)


BN_FWD = [("f32", 64, 56, 2680, "relu", "v4"), ("f32", 64, 56, 2680, "none", "v4"), ("f32", 64, 56, 2680, "add_relu", "v4"),
          ("f32", 2048, 7, 5353, "relu", "v4,straddle"), ("f32", 2047, 7, 5357, "relu", "v1"),
          ("bf16", 128, 56, 2680, "relu", "v8"), ("bf16", 128, 56, 2680, "add_relu", "v8"), ("bf16", 2048, 7, 10703, "relu", "v8,straddle")]


@pytest.mark.parametrize("case", BN_FWD, ids=["%s_C%d_H%d_%s" % (c[0], c[1], c[2], c[4]) for c in BN_FWD])
def test_e_bn_forward_past_2_gib(L, case):
    """mi_op_bn_fwd_t (sparse input): statistics over all N images against float64, every apply form on the slab images with the kernel's own
    statistics -- among them the 7x7 planes whose vectors straddle two channels and the scalar form of an odd tensor -- and, for the
    "relu" form, mi_op_bn_apply_t from the same statistics bit for bit"""
    pair, Cn, H, N, form, vec = case
    dt = BF16 if pair == "bf16" else F32
    bf = dt == BF16
    N, Cn, H, Ei, S = _ew_geometry(dt, Cn, H, N)
    gamma, beta = _bn_vectors(Cn, Cn + 1)
    xs = slab_data(S, (Cn, H, H), Cn + 2, bf) * np.float32(0.5) + np.float32(0.25)
    xs = R.bf16_round32(xs) if bf else xs
    with Case(L, "bn fwd %s C%d H%d N%d %s" % (pair, Cn, H, N, form)) as c:
        a = c.a
        x = a.new_zero(N * Ei, dt)
        a.write_images(x, S, Ei, xs, dt)
        res = a.new_filled(N * Ei, 31, 0.0, 1.0, dt) if form == "add_relu" else None
        y = a.new_poisoned(N * Ei, dt)
        gd, bd, md, vd = a.upload(gamma), a.upload(beta), a.new_poisoned(Cn), a.new_poisoned(Cn)
        c.ok(c.run("mi_op_bn_fwd_t", x, dt, gd, bd, res, md, vd, y, dt, N, Cn, H, EPS, int(form == "relu")), c.name)
        G.assert_launched(L, ["bn_stats_kernel", "bn_finalize_kernel", "bn_apply_kernel<%s,%s,%s>" % (pair, pair, vec)], c.name)
        gm, gv = a.download(md, Cn), a.download(vd, Cn)
        bad, ws = G.stats_distance(gm, gv, G.sparse_bn_stats(xs, N * H * H))
        assert bad == 0, "statistics: %d values out of bounds (worst %.3g x 2^-24)" % (bad, ws)
        rs = G.regen_images(31, 0.0, 1.0, S, Ei, dt).reshape(xs.shape) if res else None
        ref, A = E.apply_ref(xs, gamma, beta, gm, gv, EPS, form != "none", rs)
        got = a.read_images(y, S, Ei, dt).reshape(xs.shape)
        c.check(got, ref, A, bf, "images %s" % (S,))
        if form == "relu":
            y2 = a.new_poisoned(N * Ei, dt)
            c.ok(c.run("mi_op_bn_apply_t", x, dt, gd, bd, None, md, vd, y2, dt, N, Cn, H, EPS, 1), "mi_op_bn_apply_t")
            G.assert_launched(L, ["bn_apply_kernel<%s,%s,%s>" % (pair, pair, vec)], "mi_op_bn_apply_t")
            c.exact(a.read_images(y2, S, Ei, dt).reshape(xs.shape), got, "mi_op_bn_apply_t against the forward's output")
        c.worst = max(c.worst, ws)


@pytest.mark.parametrize("par", [0, 1], ids=["plane", "parity"])
def test_e_bn_forward_channel_last_bf16_past_2_gib(L, par):
    """mi_op_bn_fwd_cl_bf16, 128 channels @56 at N = 2680: y on the slab images, and the channel-last copy of those images (one padded plane,
    or the four parity planes) bit for bit, halos zero"""
    N, Cn, H, Ei, S = _ew_geometry(BF16)
    gamma, beta = _bn_vectors(Cn, 41)
    xs = R.bf16_round32(slab_data(S, (Cn, H, H), 42, True) * np.float32(0.5) + np.float32(0.25))
    Ecl = (4 * (H // 2 + 1) ** 2 if par else (H + 2) ** 2) * Cn
    with Case(L, "bn fwd cl bf16 C%d H%d N%d %s" % (Cn, H, N, "parity planes" if par else "plane")) as c:
        a = c.a
        x = a.new_zero(N * Ei, BF16)
        a.write_images(x, S, Ei, xs, BF16)
        y, ycl = a.new_poisoned(N * Ei, BF16), a.new_zero(N * Ecl, BF16)
        gd, bd, md, vd = a.upload(gamma), a.upload(beta), a.new_poisoned(Cn), a.new_poisoned(Cn)
        c.ok(c.run("mi_op_bn_fwd_cl_bf16", x, gd, bd, None, md, vd, y, ycl, N, Cn, H, EPS, par), c.name)
        G.assert_launched(L, ["bn_stats_kernel", "bn_apply_cl_kernel"], c.name)
        gm, gv = a.download(md, Cn), a.download(vd, Cn)
        bad, ws = G.stats_distance(gm, gv, G.sparse_bn_stats(xs, N * H * H))
        assert bad == 0, "statistics: %d values out of bounds (worst %.3g x 2^-24)" % (bad, ws)
        ref, A = E.apply_ref(xs, gamma, beta, gm, gv, EPS, True)
        got = a.read_images(y, S, Ei, BF16).reshape(xs.shape)
        c.check(got, ref, A, True, "images %s" % (S,))
        cl = a.read_images(ycl, S, Ecl, BF16)
        c.exact(cl.reshape(E.channel_last(got, bool(par)).shape), E.channel_last(got, bool(par)), "the channel-last copy")


BN_BWD = [(pair, None, EW_H, EW_N, mode, "v8" if pair == "bf16" else "v4") for pair in ("f32", "bf16") for mode in (0, 1, 3)] + \
         [("f32", 2048, 7, 5353, 3, "v4,straddle"), ("bf16", 2048, 7, 10703, 0, "v8,straddle")]


@pytest.mark.parametrize("case", BN_BWD, ids=["%s_C%s_H%d_mode%d" % (c[0], c[1] or "ew", c[2], c[4]) for c in BN_BWD])
def test_e_bn_backward_past_2_gib(L, case):
    """mi_op_bn_bwd_t (sparse dY; given statistics): dbeta and dgamma against float64 sums of the gated gradient, dx on the slab images,
    mode 3's gated dY bit for bit.  Mode 1 recomputes the gate from y > 0: the slab images of x hold values a 64th apart around a mean
    between two of them, beta = 0, so that no y lies near the gate's edge.  The 7x7 cases take the apply pass whose vectors straddle two
    channels"""
    pair, Cn, H, N, mode, vec = case
    dt = BF16 if pair == "bf16" else F32
    bf = dt == BF16
    N, Cn, H, Ei, S = _ew_geometry(dt, Cn, H, N)
    shp = (len(S), Cn, H, H)
    gamma, beta = _bn_vectors(Cn, 51 + mode)
    rng = np.random.default_rng(52 + mode)
    means = R.bf16_round32(rng.uniform(-0.2, 0.2, Cn).astype(np.float32))
    vars_ = rng.uniform(0.2, 0.5, Cn).astype(np.float32)
    dys = slab_data(S, (Cn, H, H), 53 + mode, bf)
    with Case(L, "bn bwd %s C%d H%d N%d mode %d" % (pair, Cn, H, N, mode)) as c:
        a = c.a
        dy = a.new_zero(N * Ei, dt)
        a.write_images(dy, S, Ei, dys, dt)
        x = a.new_filled(N * Ei, 54, -1.0, 1.0, dt)
        xs = G.regen_images(54, -1.0, 1.0, S, Ei, dt).reshape(shp)
        if mode == 1:
            beta[:] = 0
            means[:] = np.float32(1.0 / 128)
            xs = (np.rint(xs * 64) / 64).astype(np.float32)
            a.write_images(x, S, Ei, xs, dt)
        mask = a.new_filled(N * Ei, 55, -1.0, 1.0, dt) if mode == 3 else None
        gated = a.new_poisoned(N * Ei, dt) if mode == 3 else None
        dx = a.new_poisoned(N * Ei, dt)
        gd, bd, md, vd = a.upload(gamma), a.upload(beta), a.upload(means), a.upload(vars_)
        dg, db = a.new_poisoned(Cn), a.new_poisoned(Cn)
        c.ok(c.run("mi_op_bn_bwd_t", x, dt, gd, bd, md, vd, dy, mask, gated, dt, dx, dg, db, N, Cn, H, EPS, mode), c.name)
        G.assert_launched(L, ["bn_bwd_reduce_kernel", "bn_bwd_finalize_kernel", "bn_bwd_apply_kernel<%s,%s,%s>" % (pair, pair, vec)], c.name)
        if mode == 0:
            g = dys
        elif mode == 1:
            yv, bound = E.bn_gate_y(xs, gamma, beta, means, vars_, EPS)
            assert not np.any(np.abs(yv) <= 2 * bound), "an element at the gate's edge"
            g = np.where(yv > 0, dys, np.float32(0))
        else:
            g = np.where(G.regen_images(55, -1.0, 1.0, S, Ei, dt).reshape(shp) > 0, dys, np.float32(0))
            c.exact(a.read_images(gated, S, Ei, dt).reshape(shp), g, "mode 3's gated dY")
        sums = E.grad_sums(g, xs, means, vars_, EPS)
        bad, ws = E.sums_violations(a.download(db, Cn), a.download(dg, Cn), sums)
        assert bad == 0, "dbeta / dgamma: %d values out of bounds (worst %.3g x 2^-24 sum|terms|)" % (bad, ws)
        ref, A = E.dx_ref(g, xs, gamma, means, vars_, EPS, sums, N * H * H)
        c.check(a.read_images(dx, S, Ei, dt).reshape(shp), ref, A, bf, "dx, images %s" % (S,))
        c.worst = max(c.worst, ws)


def test_e_relu_deriv_and_convert_past_2_gib(L):
    """mi_op_relu_deriv on 2680 x 200704 floats; mi_op_convert fp32 -> bf16 -> fp32 on twice the elements (the fp32 side passes 2^32 bytes)"""
    N, Cn, H, Ei, S = _ew_geometry(F32)
    with Case(L, "relu_deriv N%d x %d" % (N, Ei)) as c:
        a = c.a
        x, up, out = a.new_filled(N * Ei, 61, -1.0, 1.0), a.new_filled(N * Ei, 62, -1.0, 1.0), a.new_poisoned(N * Ei)
        c.ok(c.run("mi_op_relu_deriv", x, up, out, N * Ei), c.name)
        G.assert_launched(L, ["relu_deriv_kernel"], c.name)
        xs, us = G.regen_images(61, -1.0, 1.0, S, Ei), G.regen_images(62, -1.0, 1.0, S, Ei)
        c.exact(a.read_images(out, S, Ei), np.where(xs > 0, us, np.float32(0)), "images %s" % (S,))
    N, Cn, H, Ei, S = _ew_geometry(BF16)
    S = sorted(set(S) | set(G.boundary_images(N, Ei, 4, 3, 0)))
    with Case(L, "convert N%d x %d" % (N, Ei)) as c:
        a = c.a
        src, bfp, back = a.new_filled(N * Ei, 63, -1.0, 1.0), a.new_poisoned(N * Ei, BF16), a.new_poisoned(N * Ei)
        c.ok(c.run("mi_op_convert", src, F32, bfp, BF16, N * Ei), "fp32 -> bf16")
        G.assert_launched(L, ["bg_f2b_kernel"], c.name)
        want = G.regen_images(63, -1.0, 1.0, S, Ei, BF16)
        c.exact(a.read_images(bfp, S, Ei, BF16), want, "fp32 -> bf16, images %s" % (S,))
        c.ok(c.run("mi_op_convert", bfp, BF16, back, F32, N * Ei), "bf16 -> fp32")
        G.assert_launched(L, ["bg_b2f_kernel"], c.name)
        c.exact(a.read_images(back, S, Ei), want, "bf16 -> fp32, images %s" % (S,))


def test_e_nhwc_to_nchw_past_2_gib(L):
    N, Cn, H, Ei, S = _ew_geometry(F32)
    with Case(L, "nhwc_to_nchw N%d H%d C%d" % (N, H, Cn)) as c:
        a = c.a
        src, out = a.new_filled(N * Ei, 71, -1.0, 1.0), a.new_poisoned(N * Ei)
        c.ok(c.run("mi_op_nhwc_to_nchw", src, out, N, H, H, Cn), c.name)
        G.assert_launched(L, ["nhwc_to_nchw_kernel"], c.name)
        want = G.regen_images(71, -1.0, 1.0, S, Ei).reshape(len(S), H * H, Cn).transpose(0, 2, 1)
        c.exact(a.read_images(out, S, Ei).reshape(len(S), Cn, H * H), np.ascontiguousarray(want), "images %s" % (S,))


@pytest.mark.parametrize("pair", ["f32", "bf16"])
def test_e_pooling_past_2_gib(L, pair):
    """the max-pool (3x3 / 2) forward and backward and the average pool forward and backward on 2680 images of 64 (bf16: 128) channels @56:
    values, arg-max indices and both gradients on the slab images, by ewref's restated rules"""
    dt = BF16 if pair == "bf16" else F32
    N, Cn, H, Ei, S = _ew_geometry(dt)
    Ho = H // 2
    Eo = Cn * Ho * Ho
    with Case(L, "maxpool %s C%d H%d N%d" % (pair, Cn, H, N)) as c:
        a = c.a
        x, dy = a.new_filled(N * Ei, 81, -1.0, 1.0, dt), a.new_filled(N * Eo, 82, -1.0, 1.0, dt)
        y, idx, dx = a.new_poisoned(N * Eo, dt), a.alloc(N * Eo), a.new_poisoned(N * Ei, dt)
        c.ok(c.run("mi_op_maxpool_fwd_t", x, y, dt, idx, N, Cn, H, 3, 2), "max-pool forward")
        G.assert_launched(L, ["maxpool_fwd_3x3s2_kernel"], c.name)
        c.ok(c.run("mi_op_maxpool_bwd_t", idx, dy, dx, dt, N, Cn, H, 3, 2), "max-pool backward")
        G.assert_launched(L, ["maxpool_bwd_3x3s2_kernel"], c.name)
        for n in S:
            xs = G.regen(81, -1.0, 1.0, n * Ei, Ei, dt).reshape(1, Cn, H, H)
            ry, ridx = E.maxpool_fwd_ref(xs)
            c.exact(a.read(y, n * Eo, Eo, dt).reshape(ry.shape), ry, "values of image %d" % n)
            gi = a.read(idx, n * Eo, Eo, "i32").reshape(ridx.shape)
            assert np.array_equal(gi, ridx + np.int32(n * Ei)), "arg-max indices of image %d: %d differ" % (n, np.count_nonzero(gi != ridx + n * Ei))
            dys = G.regen(82, -1.0, 1.0, n * Eo, Eo, dt).reshape(1, Cn, Ho, Ho)
            c.exact(a.read(dx, n * Ei, Ei, dt).reshape(xs.shape), E.maxpool_bwd_ref(ridx, dys, H), "dx of image %d" % n)
    with Case(L, "avgpool %s C%d H%d N%d" % (pair, Cn, H, N)) as c:
        a = c.a
        x, dyp = a.new_filled(N * Ei, 83, -1.0, 1.0, dt), a.new_filled(N * Cn, 84, -1.0, 1.0)
        y, dx = a.new_poisoned(N * Cn), a.new_poisoned(N * Ei, dt)
        c.ok(c.run("mi_op_avgpool_fwd_t", x, dt, y, N, Cn, H), "average pool forward")
        G.assert_launched(L, ["avgpool_fwd_kernel"], c.name)
        c.ok(c.run("mi_op_avgpool_bwd_t", dyp, dx, dt, N, Cn, H), "average pool backward")
        G.assert_launched(L, ["avgpool_bwd_kernel"], c.name)
        xs = G.regen_images(83, -1.0, 1.0, S, Ei, dt).reshape(len(S), Cn, H, H)
        ref, A = E.avgpool_ref(xs)
        c.check(a.read_images(y, S, Cn), ref, A, False, "forward, images %s" % (S,))
        d = G.regen_images(84, -1.0, 1.0, S, Cn)
        want = np.broadcast_to((d / np.float32(H * H))[:, :, None, None], xs.shape).astype(np.float32)
        c.exact(a.read_images(dx, S, Ei, dt).reshape(xs.shape), R.bf16_round32(want) if dt == BF16 else want, "backward, images %s" % (S,))


ARENA = (1 << 29) + (1 << 20)
RUNS = [(0, 4096), ((1 << 29) - 2048, 4096), (ARENA - 4096, 4096)]   # the start, across byte 2^31, the end


def test_e_adam_past_2_gib(L):
    """mi_op_adam on an arena of 2^29 + 2^20 floats: runs at the start, across byte offset 2^31 and at the end against ewref.adam_ref"""
    hp = dict(lr=1e-3, wd=1e-4, b1=0.9, b2=0.999, cb1=0.9 ** 3, cb2=0.999 ** 3, eps=1e-8)
    with Case(L, "adam %d floats" % ARENA) as c:
        a = c.a
        p, g = a.new_filled(ARENA, 91, -1.0, 1.0), a.new_filled(ARENA, 92, -0.1, 0.1)
        m, v = a.new_filled(ARENA, 93, -0.01, 0.01), a.new_filled(ARENA, 94, 0.0, 0.01)
        flag = a.upload(np.zeros(1, np.int32), np.int32)
        c.ok(c.run("mi_op_adam", p, g, m, v, ARENA, hp["lr"], hp["wd"], hp["b1"], hp["b2"], hp["cb1"], hp["cb2"], hp["eps"], flag), c.name)
        G.assert_launched(L, ["adam_kernel"], c.name)
        assert a.download(flag, 1, np.int32)[0] == 0
        for start, n in RUNS:
            old = [G.regen(sd, lo, hi, start, n) for sd, lo, hi in ((91, -1.0, 1.0), (92, -0.1, 0.1), (93, -0.01, 0.01), (94, 0.0, 0.01))]
            for (ref, A), ptr, name in zip(E.adam_ref(*old, **hp), (p, m, v), "pmv"):
                c.check(a.read(ptr, start, n), ref, A, False, "%s[%d : %d]" % (name, start, start + n))


@pytest.mark.parametrize("kind", ["sgd", "lars"])
def test_e_momentum_update_past_2_gib(L, kind):
    """mi_op_momentum_update on the same arena as three tensors -- one of 2^29 - 2048 floats, one of 4096 across byte offset 2^31, the rest --
    against optim_ref.step with test_gpu_optim.py's bounds (rel-L2 1e-6, max-abs 2e-6 of the largest reference value), the squared norms
    of the two small tensors to 1e-6; of the large tensor, its first and last 4096 elements (LARS: with the trust ratio of its true norms,
    which the kernel's own double sums give to 1e-6 and the test takes from the uniform fill's moments)"""
    offs = [0, (1 << 29) - 2048, (1 << 29) + 2048, ARENA]
    isw = [1, 1, 0]
    kd = {"sgd": optim_ref.SGD, "lars": optim_ref.LARS}[kind]
    lr, wd, mu, tau = float(np.float32(0.5 if kind == "lars" else 0.01)), float(np.float32(5e-5)), float(np.float32(0.9)), float(np.float32(0.001))
    fills = ((95, -1.0, 1.0), (96, -0.1, 0.1), (97, -0.01, 0.01))
    with Case(L, "momentum %s %d floats" % (kind, ARENA)) as c:
        a = c.a
        p, g, b = (a.new_filled(ARENA, sd, lo, hi) for sd, lo, hi in fills)
        flag = a.upload(np.zeros(1, np.int32), np.int32)
        off = np.ascontiguousarray(offs, np.uint64)
        iw = np.ascontiguousarray(isw, np.int32)
        sq = np.zeros((3, 2), np.float64)
        c.ok(c.run("mi_op_momentum_update", kd, p, g, b, ARENA, off.ctypes.data, 3, iw.ctypes.data, lr, wd, mu, tau, flag,
                   sq.ctypes.data if kind == "lars" else None), c.name)
        G.assert_launched(L, ["optim_update_kernel"] + (["optim_norm_kernel", "optim_trust_kernel"] if kind == "lars" else []), c.name)
        assert a.download(flag, 1, np.int32)[0] == 0

        def check(start, n, tensor, what):
            w0, g0, b0 = (G.regen(sd, lo, hi, start, n) for sd, lo, hi in fills)
            s = sq[tensor] if kind == "lars" else None
            # a slab of the large tensor: LARS takes the tensor's trust ratio, which optim_ref derives from the whole tensor's norms
            if s is not None and n != offs[tensor + 1] - offs[tensor]:
                t = optim_ref.trust_ratio(s[0], s[1], wd, tau)
                rb = mu * b0.astype(np.float64) + lr * t * (g0.astype(np.float64) + wd * w0.astype(np.float64))
                rw = w0.astype(np.float64) - rb
            else:
                rw, _, rb, fl = optim_ref.step(kd, [w0], [g0], [b0], [isw[tensor]], lr, wd, mu, tau)
                rw, rb = rw[0], rb[0]
                assert fl == 0
                if kind == "lars":
                    ref_sq = optim_ref.sq_norms([w0], [g0])[0]
                    assert np.all(np.abs(s - ref_sq) <= 1e-6 * ref_sq), "squared norms of tensor %d: %s against %s" % (tensor, s, ref_sq)
            for name, ptr, ref in (("w", p, rw), ("b", b, rb)):
                got = a.read(ptr, start, n).astype(np.float64)
                rel = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
                mx, scale = float(np.max(np.abs(got - ref))), float(np.max(np.abs(ref)))
                assert rel <= 1e-6 and mx <= 2e-6 * scale, "%s %s: rel-L2 %.3e, max-abs %.3e (max|ref| %.3e)" % (what, name, rel, mx, scale)
                c.worst, c.unit = max(c.worst, rel), "rel-L2"
            assert not np.any(a.read(g, start, n)), "%s: the gradient is not cleared" % what

        check(offs[1], 4096, 1, "the tensor across byte 2^31")
        check(offs[2], offs[3] - offs[2], 2, "the tensor past it")
        check(0, 4096, 0, "the start of the large tensor")
        check(offs[1] - 4096, 4096, 0, "the end of the large tensor")
        if kind == "lars":  # the large tensor's norms: uniform(-1, 1) and (-0.1, 0.1) over 2^29 - 2048 elements, E[x^2] = hi^2 / 3 to 1e-3
            n0 = offs[1]
            assert abs(sq[0, 0] / (n0 / 3.0) - 1) < 1e-3 and abs(sq[0, 1] / (n0 * 0.01 / 3.0) - 1) < 1e-3, sq[0]


def test_e_loss_head_past_2_gib(L):
    """mi_op_loss_head at N * L > 2^29 (536888 rows of 1000): pred against ewref.softmax_ref, dlogits = pred - onehot bit for bit (no
    smoothing), the row loss inside lossref.loss_bound and the rank by lossref's rule on the device's own pred -- on rows at the start,
    across byte offset 2^31 and at the end"""
    Ln = 1000
    N = (1 << 29) // Ln + 18
    rows = [(0, 8), ((1 << 29) // Ln - 4, 8), (N - 8, 8)]
    with Case(L, "loss head N%d L%d" % (N, Ln)) as c:
        a = c.a
        x = a.new_filled(N * Ln, 98, -6.0, 6.0)
        lab_all = np.arange(N, dtype=np.int64) * 7 % Ln
        lab = a.upload(lab_all, np.int32)
        pred, dl = a.new_poisoned(N * Ln), a.new_poisoned(N * Ln)
        rl, rr = a.new_poisoned(N), a.alloc(N)
        c.ok(c.run("mi_op_loss_head", x, lab, pred, dl, rl, rr, N, Ln, 0.0, 5, None, None), c.name)
        G.assert_launched(L, ["loss_head_kernel<"], c.name)
        for r0, n in rows:
            xs = G.regen(98, -6.0, 6.0, r0 * Ln, n * Ln).reshape(n, Ln)
            labs = lab_all[r0:r0 + n]
            ref, A = E.softmax_ref(xs)
            got = a.read(pred, r0 * Ln, n * Ln).reshape(n, Ln)
            c.check(got, ref, A, False, "pred rows %d.." % r0)
            want = got.copy()
            want[np.arange(n), labs] -= np.float32(1)
            c.exact(a.read(dl, r0 * Ln, n * Ln).reshape(n, Ln), want, "dlogits rows %d.." % r0)
            ref_loss = lossref.loss_head(xs, labs, 0.0)[2]
            err = np.abs(a.read(rl, r0, n).astype(np.float64) - ref_loss)
            assert np.all(err <= lossref.loss_bound(ref_loss)), (r0, err, lossref.loss_bound(ref_loss))
            assert np.array_equal(a.read(rr, r0, n, "i32"), lossref.rank_of(got, labs))


# ---------------------------------------------------------------------------------------------------------------------------
# (f) 2^31 and 2^32 elements
def test_f_bn_apply_at_2_31_elements(L):
    """mi_op_bn_apply_t on 10704 x 64 @56 floats (2^31 elements and 1.3 M more, device-only operands): the 32-bit element index of the
    apply pass is exact below 2^32 (mi_common.hpp), so the kernel runs and its slab images -- the last ones lie past element 2^31 --
    are checked"""
    Cn, H = 64, 56
    Ei = Cn * H * H
    N = (1 << 31) // Ei + 5
    S = sorted(set(G.boundary_images(N, Ei, 4, 5, 0)) | {(1 << 31) // Ei - 1, (1 << 31) // Ei, (1 << 31) // Ei + 1})
    gamma, beta = _bn_vectors(Cn, 101)
    rng = np.random.default_rng(102)
    means, vars_ = rng.uniform(-0.2, 0.2, Cn).astype(np.float32), rng.uniform(0.2, 0.5, Cn).astype(np.float32)
    with Case(L, "bn apply f32 C64 H56 N%d (2^31 elements)" % N) as c:
        a = c.a
        x, y = a.new_filled(N * Ei, 103, -1.0, 1.0), a.new_poisoned(N * Ei)
        gd, bd, md, vd = a.upload(gamma), a.upload(beta), a.upload(means), a.upload(vars_)
        rc = c.run("mi_op_bn_apply_t", x, F32, gd, bd, None, md, vd, y, F32, N, Cn, H, EPS, 1)
        if rc != 0:
            G.assert_refused(L, rc, c.name)
            c.unit = "(refused)"
            return
        G.assert_launched(L, ["bn_apply_kernel<f32,f32,v4>"], c.name)
        xs = G.regen_images(103, -1.0, 1.0, S, Ei).reshape(len(S), Cn, H, H)
        ref, A = E.apply_ref(xs, gamma, beta, means, vars_, EPS, True)
        c.check(a.read_images(y, S, Ei).reshape(xs.shape), ref, A, False, "images %s" % (S,))


def test_f_bn_refuses_2_32_elements(L):
    """BN forward, apply and backward on 21400 x 64 @56 elements (past 2^32): every entry refuses, names the limit and launches nothing.
    The tensors are allocated whole (two of 17.2 GB, shared by the three calls), so that a call which did run would stay inside them"""
    Cn, H = 64, 56
    Ei = Cn * H * H
    N = (1 << 32) // Ei + 1
    assert N * Ei >= 1 << 32
    with Case(L, "bn f32 C64 H56 N%d (2^32 elements)" % N) as c:
        a = c.a
        x, y = a.alloc(N * Ei), a.alloc(N * Ei)
        v = [a.new_filled(Cn, 110 + i, 0.5, 1.0) for i in range(6)]
        G.assert_refused(L, c.run("mi_op_bn_fwd_t", x, F32, v[0], v[1], None, v[2], v[3], y, F32, N, Cn, H, EPS, 1), "mi_op_bn_fwd_t")
        G.assert_refused(L, c.run("mi_op_bn_apply_t", x, F32, v[0], v[1], None, v[2], v[3], y, F32, N, Cn, H, EPS, 1), "mi_op_bn_apply_t")
        G.assert_refused(L, c.run("mi_op_bn_bwd_t", x, F32, v[0], v[1], v[2], v[3], x, None, None, F32, y, v[4], v[5], N, Cn, H, EPS, 0), "mi_op_bn_bwd_t")
        c.unit = "(refused)"


def test_f_pooling_at_2_31_elements(L):
    """10704 x 64 @56 floats: the max-pool refuses in both directions (its arg-max indices are 32-bit ints) and names the limit; the
    average pool indexes with 64 bits and runs"""
    Cn, H = 64, 56
    Ei, Eo = Cn * H * H, Cn * (H // 2) ** 2
    N = (1 << 31) // Ei + 5
    S = sorted(set(G.boundary_images(N, Ei, 4, 6, 0)) | {(1 << 31) // Ei, (1 << 31) // Ei + 1})
    with Case(L, "pooling f32 C64 H56 N%d (2^31 elements)" % N) as c:
        a = c.a
        x, big = a.new_filled(N * Ei, 120, -1.0, 1.0), a.alloc(N * Ei)
        y, idx = a.alloc(N * Eo), a.alloc(N * Eo)
        G.assert_refused(L, c.run("mi_op_maxpool_fwd_t", x, y, F32, idx, N, Cn, H, 3, 2), "mi_op_maxpool_fwd_t")
        G.assert_refused(L, c.run("mi_op_maxpool_bwd_t", idx, y, big, F32, N, Cn, H, 3, 2), "mi_op_maxpool_bwd_t")
        pooled = a.new_poisoned(N * Cn)
        c.ok(c.run("mi_op_avgpool_fwd_t", x, F32, pooled, N, Cn, H), "average pool forward")
        G.assert_launched(L, ["avgpool_fwd_kernel"], c.name)
        xs = G.regen_images(120, -1.0, 1.0, S, Ei).reshape(len(S), Cn, H, H)
        ref, A = E.avgpool_ref(xs)
        c.check(a.read_images(pooled, S, Cn), ref, A, False, "average pool forward, images %s" % (S,))
        c.ok(c.run("mi_op_avgpool_bwd_t", pooled, big, F32, N, Cn, H), "average pool backward")
        G.assert_launched(L, ["avgpool_bwd_kernel"], c.name)
        d = a.read_images(pooled, S, Cn)
        want = np.broadcast_to((d / np.float32(H * H))[:, :, None, None], xs.shape).astype(np.float32)
        c.exact(a.read_images(big, S, Ei).reshape(xs.shape), want, "average pool backward, images %s" % (S,))


def test_the_device_fill_is_the_stream_largeref_restates(L):
    """mi_op_fill_uniform and mi_op_convert on a small tensor against largeref.regen, run by run (what every case above rests on)"""
    n = 100003
    with Case(L, "fill against regen") as c:
        a = c.a
        p, q = a.new_filled(n, 7, -1.0, 1.0), a.new_filled(n + 1, 7, -3.0, 5.0, BF16)
        c.exact(a.read(p, 0, n), G.regen(7, -1.0, 1.0, 0, n), "fp32")
        c.exact(a.read(p, 77777, 1000), G.regen(7, -1.0, 1.0, 77777, 1000), "fp32 run")
        c.exact(a.read(q, 5, n - 5, BF16), G.regen(7, -3.0, 5.0, 5, n - 5, BF16), "bf16")
        z, nn = a.new_zero(64, BF16), a.new_poisoned(64, BF16)
        assert not np.any(a.read(z, 0, 64, BF16)) and np.all(np.isnan(a.read(nn, 0, 64, BF16)))
        a.write(q, 10, np.arange(8, dtype=np.float32) * np.float32(1.001), BF16)
        c.exact(a.read(q, 10, 8, BF16), R.bf16_round32(np.arange(8, dtype=np.float32) * np.float32(1.001)), "bf16 write")
