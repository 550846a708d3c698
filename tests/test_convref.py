"""The checker of test_gpu_batch256.py on the CPU (no GPU): it accepts correct float32 results however they are summed, rejects
results that are subtly wrong, and the batch-256 case list reaches every kind of launch plan (mi_conv_plan, host-only)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convref as R

N = 4
SHAPES = [c[:5] for c in R.LAYERS]
SIDS = ["C%d_H%d_K%d_k%d_s%d" % s for s in SHAPES]


@pytest.fixture(scope="module", autouse=True)
def _threads():
    R.set_threads(16)


def _data(shape, bf=False):
    Cn, H, K, k, s = shape
    rng = np.random.default_rng(Cn * 7 + H * 3 + K + k + s)
    f = R.bf16_round32 if bf else (lambda a: a)
    x = f(rng.standard_normal((N, Cn, H, H), dtype=np.float32))
    w = f((rng.standard_normal((K, Cn, k, k), dtype=np.float32) * np.float32((2.0 / (k * k * (Cn + K))) ** 0.5)))
    dy = f(rng.standard_normal((N, K, H // s, H // s), dtype=np.float32))
    return x, w, dy


def _f32(op, x, w, dy, shape):
    """torch float32 CPU"""
    Cn, H, K, k, s = shape
    t = torch.from_numpy
    if op == "fwd":
        return F.conv2d(t(x), t(w), stride=s, padding=k // 2).numpy()
    if op == "dgrad":
        Ho = H // s
        return F.conv_transpose2d(t(dy), t(w), stride=s, padding=k // 2, output_padding=H - ((Ho - 1) * s - 2 * (k // 2) + k)).numpy()
    return torch.nn.grad.conv2d_weight(t(x), w.shape, t(dy), stride=s, padding=k // 2).numpy()


def _f32_blocked(op, x, w, dy, shape):
    """float32, summed in another order: per 64-channel block of the reduction, blocks added one after another in float32
    (the weight gradient: per image, images added in reverse order)"""
    Cn, H, K, k, s = shape
    if op == "fwd":
        out = None
        for c0 in range(0, Cn, 64):
            p = _f32(op, x[:, c0:c0 + 64], w[:, c0:c0 + 64], dy, (min(64, Cn - c0), H, K, k, s))
            out = p if out is None else (out + p).astype(np.float32)
        return out
    if op == "dgrad":
        out = None
        for k0 in range(0, K, 64):
            p = _f32(op, x, w[k0:k0 + 64], dy[:, k0:k0 + 64], (Cn, H, min(64, K - k0), k, s))
            out = p if out is None else (out + p).astype(np.float32)
        return out
    out = None
    for n in reversed(range(N)):
        p = _f32(op, x[n:n + 1], w, dy[n:n + 1], shape)
        out = p if out is None else (out + p).astype(np.float32)
    return out


def _slabs(op, x, w, dy, shape, addend=None):
    Cn, H, K, k, s = shape
    if op == "fwd":
        return R.fwd_slabs(x, w, s, R.slab_images(N), R.slab_channels(K))
    if op == "dgrad":
        return R.dgrad_slabs(w, dy, H, s, R.slab_images(N), R.slab_channels(Cn), addend)
    return R.wgrad_slabs(x, dy, k, s, R.slab_channels(K), R.slab_channels(Cn, 1))


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SIDS)
@pytest.mark.parametrize("op", ["fwd", "dgrad", "wgrad"])
def test_no_false_alarms(shape, op):
    """torch's float32 convolution and a float32 sum in blocked order pass; with bf16 operands so do both rounded with RNE"""
    for bf in (False, True):
        x, w, dy = _data(shape, bf)
        slabs = _slabs(op, x, w, dy, shape)
        out_bf = bf and op != "wgrad"  # weight gradients stay fp32 on every route
        for got in (_f32(op, x, w, dy, shape), _f32_blocked(op, x, w, dy, shape)):
            if out_bf:
                got = R.bf16_round32(got)
            R.check_slabs(got, slabs, out_bf, "%s %s bf16=%d" % (op, shape, bf))


def test_no_false_alarm_with_addend():
    shape = (256, 14, 64, 1, 1)
    x, w, dy = _data(shape)
    addend = np.random.default_rng(5).standard_normal(x.shape, dtype=np.float32)
    got = (_f32("dgrad", x, w, dy, shape) + addend).astype(np.float32)
    R.check_slabs(got, _slabs("dgrad", x, w, dy, shape, addend), False, "dgrad + addend")
    assert R.violations(_f32("dgrad", x, w, dy, shape), _slabs("dgrad", x, w, dy, shape, addend), False) > 0


def test_bf16_rounding_is_exact():
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -40, 3.0e-3, 0.0])
    assert list(R.rne_bf16(a)) == [1.0, 1.0, 1.0 + 2 ** -6, -1.0, 1.0 + 2 ** -7, float(R.bf16_round32(np.array([3.0e-3], np.float32))[0]), 0.0]


# ---------------------------------------------------------------------------------------------------------------------------
# mutants: each applied to a correct float32 result, each must be rejected
MUTANT_SHAPES = [(128, 28, 128, 3, 1), (256, 28, 256, 3, 2), (1024, 14, 256, 1, 1), (64, 56, 64, 3, 1), (512, 7, 2048, 1, 1)]


def _median_term(terms):
    a = np.abs(terms).ravel()
    return int(np.argsort(a)[len(a) // 2])


@pytest.mark.parametrize("shape", MUTANT_SHAPES, ids=["C%d_H%d_K%d_k%d_s%d" % s for s in MUTANT_SHAPES])
def test_mutant_one_missing_term(shape):
    """1: one output in S (image N - 1) or R (a checked channel) misses one (channel, tap) term -- fwd and dgrad"""
    Cn, H, K, k, s = shape
    x, w, dy = _data(shape)
    p, Ho = k // 2, H // s
    # fwd: y[n, o, h, v] = sum_c,r,q x[n, c, h s - p + r, v s - p + q] w[o, c, r, q]; an interior output
    for (n, o) in ((N - 1, 5), (1, R.slab_channels(K)[3])):
        h = v = Ho // 2
        rows = x[n, :, h * s - p:h * s - p + k, v * s - p:v * s - p + k]
        terms = rows * w[o]
        j = _median_term(terms)
        got = _f32("fwd", x, w, dy, shape)
        got[n, o, h, v] -= terms.ravel()[j]
        assert R.violations(got, _slabs("fwd", x, w, dy, shape), False) > 0, ("fwd", n, o)
    if s == 1:  # dgrad: dx[n, c, h, v] = sum_o,r,q dy[n, o, h + p - r, v + p - q] w[o, c, r, q]
        n, c = N - 1, R.slab_channels(Cn)[2]
        h = v = H // 2
        win = dy[n, :, h + p - k + 1:h + p + 1, v + p - k + 1:v + p + 1][:, ::-1, ::-1]
        terms = win * w[:, c]
        got = _f32("dgrad", x, w, dy, shape)
        got[n, c, h, v] -= terms.ravel()[_median_term(terms)]
        assert R.violations(got, _slabs("dgrad", x, w, dy, shape), False) > 0


@pytest.mark.parametrize("shape", MUTANT_SHAPES, ids=["C%d_H%d_K%d_k%d_s%d" % s for s in MUTANT_SHAPES])
def test_mutant_bf16_truncated(shape):
    """2: one bf16 output in a slab truncated instead of rounded to nearest even"""
    x, w, dy = _data(shape, bf=True)
    for op in ("fwd", "dgrad"):
        exact = _f32(op, x, w, dy, shape)
        got = R.bf16_round32(exact)
        u = exact.view(np.uint32)
        low = u & np.uint32(0xFFFF)
        cand = np.argwhere((low > 0x9000) & (low < 0xF000))  # truncation != RNE, far from the midpoint
        cand = cand[cand[:, 0] == N - 1]
        # the largest such output: where ref is small against A (cancellation), delta exceeds a bf16 ulp and either neighbour passes
        pick = tuple(cand[np.argmax(np.abs(exact[tuple(cand.T)]))])
        got[pick] = (u[pick] & np.uint32(0xFFFF0000)).view(np.float32)
        assert R.violations(got, _slabs(op, x, w, dy, shape), True) > 0, (op, pick)


@pytest.mark.parametrize("shape", MUTANT_SHAPES, ids=["C%d_H%d_K%d_k%d_s%d" % s for s in MUTANT_SHAPES])
@pytest.mark.parametrize("how", ["lost", "twice"])
def test_mutant_wgrad_split_lost_or_duplicated(shape, how):
    """3: a weight gradient that loses one image's contribution, or counts it twice"""
    x, w, dy = _data(shape)
    one = _f32("wgrad", x[1:2], w, dy[1:2], shape)
    got = _f32("wgrad", x, w, dy, shape) + (-one if how == "lost" else one)
    assert R.violations(got.astype(np.float32), _slabs("wgrad", x, w, dy, shape), False) > 0


@pytest.mark.parametrize("shape", MUTANT_SHAPES, ids=["C%d_H%d_K%d_k%d_s%d" % s for s in MUTANT_SHAPES])
@pytest.mark.parametrize("how", ["shifted", "slice"])
def test_mutant_tile(shape, how):
    """4: one 64 x 128 tile of the output matrix (rows = output channels, columns = image pixels) at an arbitrary position shifted by
    one column, or missing one reduction slice (32 input channels, every tap)"""
    Cn, H, K, k, s = shape
    x, w, dy = _data(shape)
    Ho = H // s
    P = Ho * Ho
    got = _f32("fwd", x, w, dy, shape)
    mat = got.transpose(1, 0, 2, 3).reshape(K, N * P).copy()
    rng = np.random.default_rng(K + P)
    r0 = int(rng.integers(0, K // 64)) * 64
    c0 = int(rng.integers(0, max(1, (N * P - 128) // 128 + 1))) * 128
    c1 = min(N * P, c0 + 128)
    if how == "shifted":
        mat[r0:r0 + 64, c0:c1 - 1] = mat[r0:r0 + 64, c0 + 1:c1]
    else:
        part = _f32("fwd", x[:, 32:64], w[:, 32:64], dy, (32, H, K, k, s)).transpose(1, 0, 2, 3).reshape(K, N * P)
        mat[r0:r0 + 64, c0:c1] -= part[r0:r0 + 64, c0:c1]
    got = np.ascontiguousarray(mat.reshape(K, N, Ho, Ho).transpose(1, 0, 2, 3))
    assert R.violations(got, _slabs("fwd", x, w, dy, shape), False) > 0


@pytest.mark.parametrize("shape", MUTANT_SHAPES, ids=["C%d_H%d_K%d_k%d_s%d" % s for s in MUTANT_SHAPES])
def test_mutant_last_pixel(shape):
    """5: the last pixel of image N - 1 replaced by its neighbour"""
    x, w, dy = _data(shape)
    for op in ("fwd", "dgrad"):
        got = _f32(op, x, w, dy, shape)
        got[N - 1, :, -1, -1] = got[N - 1, :, -1, -2]
        assert R.violations(got, _slabs(op, x, w, dy, shape), False) > 0, op


# ---------------------------------------------------------------------------------------------------------------------------
def test_batch256_cases_reach_every_plan_kind():
    """the case list of test_gpu_batch256.py, planned by mi_conv_plan (host-only): it holds a mixed whole / sliced round (fp32 fwd and
    dgrad), 64- and 128-row tiles, split weight gradients >= 16 with the grouped reduce and 2..15, channel-last and LDS-DMA 1x1 weight
    gradients with splits, and both tile heights of the bf16 NCHW kernels"""
    from resnet_amd import binding as B
    L = B.load()
    kinds = set()
    print("\n%-5s %-7s %-5s %-22s %-24s %s" % ("dtype", "route", "op", "(C, H, K, k, s)", "where", "bm bn tiles full slices splits grouped"))
    for (dt, route, op, Cn, H, K, k, s, where) in R.batch256_cases(L):
        p = R.conv_plan(L, 0 if dt == "f32" else 1, route, op, R.N256, Cn, H, K, k, s)
        print("%-5s %-7s %-5s %-22s %-24s %s" % (dt, route, op, (Cn, H, K, k, s), where, p if p else "other kernels"))
        if p is None:
            assert dt == "f32" and op == "wgrad", "a bf16 route the trainer takes refuses its shape"
            continue
        bm, bn, tiles, full, slices, splits, grouped = p
        if dt == "f32" and op != "wgrad" and 0 < full < tiles and slices > 1:
            kinds.add("mixed " + op)
        if dt == "f32":
            kinds.add("bm%d" % bm)
        if op == "wgrad" and splits >= 16 and grouped:
            kinds.add("splits>=16 grouped")
        if op == "wgrad" and 2 <= splits < 16:
            kinds.add("2<=splits<16")
        if route in ("cl", "cl2", "pw") and op == "wgrad" and splits > 1:
            kinds.add(route + " wgrad split")
        if dt == "bf16" and route == "default":
            kinds.add("bf16 nchw bm%d" % bm)
    want = {"mixed fwd", "mixed dgrad", "bm64", "bm128", "splits>=16 grouped", "2<=splits<16", "cl2 wgrad split", "pw wgrad split",
            "bf16 nchw bm64", "bf16 nchw bm128"}
    assert want <= kinds, want - kinds


def test_conv_plan_refuses_and_matches_the_implicit_gemm_view():
    """mi_conv_plan: -2 where a route refuses the shape; the fp32 route reports what mi_debug_conv_plan reports"""
    import ctypes as C
    from resnet_amd import binding as B
    L = B.load()
    out = (C.c_int * 7)()
    assert L.mi_conv_plan(0, 0, 0, 256, 3, 224, 64, 7, 2, out) == -2 and list(out) == [0] * 7
    assert L.mi_conv_plan(1, 1, 0, 256, 64, 56, 256, 1, 1, out) == -2   # channel-last route: 3x3 only
    assert L.mi_conv_plan(0, 1, 0, 256, 64, 56, 64, 3, 1, out) == -2    # no channel-last route in fp32
    assert L.mi_conv_plan(1, 0, 3, 256, 64, 56, 64, 3, 1, out) == -2    # no such op
    for (Cn, H, K, k, s, _) in R.LAYERS:
        for op in range(3):
            d = (C.c_int * 9)()
            if L.mi_debug_conv_plan(op, 256, Cn, H, K, k, s, d) != 1:
                continue
            assert L.mi_conv_plan(0, 0, op, 256, Cn, H, K, k, s, out) == 0
            assert (out[0], out[2], out[3], out[4], out[5]) == (d[1], d[2], d[3], d[4], d[6])


# ---------------------------------------------------------------------------------------------------------------------------
# the case lists built from (dims, N)
def _lib():
    from resnet_amd import binding as B
    return B.load()


def test_generalized_lists_reproduce_the_batch256_lists():
    """trainer_layers / trainer_conv_cases / trainer_conv_bn_cases / trainer_dgrad_bn_cases of ResNet-50 at N = 256 are the lists the
    batch-256 file checked when they were written by hand: LAYERS, every (layer, op) in fp32 and on its bf16 route plus the 1x1 forward on a
    channel-last input, conv + BN per layer and dtype, dgrad + BN' at every reduction but b0's (fp32 and bf16) and every expansion (bf16)"""
    import synth
    L = _lib()
    assert R.trainer_layers(synth.R50_DIMS) == R.LAYERS
    want = []
    for (Cn, H, K, k, s, where) in R.LAYERS:
        for op in R.OPS:
            want.append(("f32", "default", op, Cn, H, K, k, s, where))
            want.append(("bf16", R.bf16_route(L, op, R.N256, Cn, H, K, k, s), op, Cn, H, K, k, s, where))
        if k == 1:
            want.append(("bf16", "pw", "fwd", Cn, H, K, k, s, where))
    assert R.batch256_cases(L) == want
    assert R.conv_bn_cases() == [(dt,) + layer for layer in R.LAYERS for dt in ("f32", "bf16")]
    want = []
    for layer in R.LAYERS:
        red = "red" in layer[5] and layer[5] != "b0 red"
        if red:
            want.append(("f32",) + layer)
        if red or " exp" in layer[5]:
            want.append(("bf16",) + layer)
    assert R.dgrad_bn_cases(L) == want
    # every fp32 site fuses (its dgrad runs on the implicit GEMM), every bf16 3x3 forward runs channel-last
    assert all(R.conv_plan(L, 0, "default", "dgrad", R.N256, *c[1:6]) is not None for c in want if c[0] == "f32")
    assert R.trainer_conv_bn_cl_cases(L, synth.R50_DIMS, R.N256) == [layer for layer in R.LAYERS if layer[3] == 3]


def _kinds(L, cases, N, table=None):
    """the plan kinds of test_batch256_cases_reach_every_plan_kind, plus the partial last column tile per route family and the partial tile
    inside a sliced round (fp32 fwd / dgrad); prints the table"""
    kinds, sliced_partial = set(), 0
    for (dt, route, op, Cn, H, K, k, s, where) in cases:
        p = R.conv_plan(L, 0 if dt == "f32" else 1, route, op, N, Cn, H, K, k, s)
        if table is not None:
            table.append("%-5s %-7s %-5s %-22s %-24s %s" % (dt, route, op, (Cn, H, K, k, s), where, p if p else "other kernels"))
        if p is None:
            assert dt == "f32" and op == "wgrad", "a bf16 route the trainer takes refuses its shape: %s" % ((dt, route, op, Cn, H, K, k, s),)
            continue
        bm, bn, tiles, full, slices, splits, grouped = p
        if dt == "f32" and op != "wgrad" and 0 < full < tiles and slices > 1:
            kinds.add("mixed " + op)
        if dt == "f32":
            kinds.add("bm%d" % bm)
        if op == "wgrad" and splits >= 16 and grouped:
            kinds.add("splits>=16 grouped")
        if op == "wgrad" and 2 <= splits < 16:
            kinds.add("2<=splits<16")
        if route in ("cl", "cl2", "pw") and op == "wgrad" and splits > 1:
            kinds.add(route + " wgrad split")
        if dt == "bf16" and route == "default":
            kinds.add("bf16 nchw bm%d" % bm)
        if op != "wgrad":
            P = (H // s) ** 2 if op == "fwd" else H * H
            cols = N * ((P + 7) // 8 * 8 if dt == "bf16" and route == "default" else P)
            if cols % bn:
                fam = {"f32": "f32 igemm"}.get(dt, {"default": "bf16 nchw", "cl": "channel-last", "pw": "channel-last"}[route])
                kinds.add("partial tile " + fam)
                if dt == "f32" and 0 < full < tiles and slices > 1:  # (the sliced tail round behind the whole ones holds the last tiles)
                    kinds.add("partial tile in a sliced round")
                    sliced_partial += 1
    return kinds, sliced_partial


PLAN_KINDS = {"mixed fwd", "mixed dgrad", "bm64", "bm128", "splits>=16 grouped", "2<=splits<16", "cl2 wgrad split", "pw wgrad split",
              "bf16 nchw bm64", "bf16 nchw bm128"}


def test_batch33_cases_reach_every_plan_kind_and_partial_tiles():
    """ResNet-50 at N = 33 (test_gpu_ragged.py): every plan kind of the batch-256 list, a partial last column tile on every fwd / dgrad
    case (the fp32 implicit GEMM, the bf16 NCHW and the channel-last kernels), and partial tiles inside sliced rounds -- none of which N = 256
    has"""
    import synth
    L = _lib()
    table = []
    kinds, nsp = _kinds(L, R.trainer_conv_cases(L, synth.R50_DIMS, 33), 33, table)
    print("\nResNet-50 at N = 33\n%-5s %-7s %-5s %-22s %-24s %s" % ("dtype", "route", "op", "(C, H, K, k, s)", "where",
                                                                 "bm bn tiles full slices splits grouped"))
    print("\n".join(table))
    print("kinds: %s; fp32 fwd / dgrad cases with the partial tile inside a sliced tail round: %d" % (sorted(kinds), nsp))
    want = PLAN_KINDS | {"partial tile f32 igemm", "partial tile bf16 nchw", "partial tile channel-last", "partial tile in a sliced round"}
    assert want <= kinds, want - kinds
    k256, n256 = _kinds(L, R.batch256_cases(L), R.N256)
    assert not any(k.startswith("partial") for k in k256) and n256 == 0, "N = 256 fills every column tile"
    # every fp32 / bf16 fwd and dgrad of the 256 list ends in a partial tile at N = 33
    for (dt, route, op, Cn, H, K, k, s, where) in R.trainer_conv_cases(L, synth.R50_DIMS, 33):
        if op == "wgrad" or route == "pw" or dt == "f32" and R.conv_plan(L, 0, route, op, 33, Cn, H, K, k, s) is None:
            continue
        p = R.conv_plan(L, 0 if dt == "f32" else 1, route, op, 33, Cn, H, K, k, s)
        P = (H // s) ** 2 if op == "fwd" else H * H
        assert 33 * ((P + 7) // 8 * 8 if dt == "bf16" and route == "default" else P) % p[1], (dt, route, op, Cn, H, K, k, s)


def test_trajectory_nets_hold_their_trainers_routes():
    """C1S and C4I at N = 4, ResNet-50 at N = 8 (test_gpu_trajectory.py's nets and batches): every convolution of plan_layers is in the
    list in fp32 and on the bf16 route the planner gives it, every route the list names plans the shape, and the 3x3 layers run channel-last
    on the 8 x 8 and 4 x 4 planes"""
    L = _lib()
    for net, N in (("c1s", 4), ("c4i", 4), ("r50", 8)):
        d = R.nets()[net]
        cases = R.trainer_conv_cases(L, d, N)
        shapes = {u[2] for u in R.trainer_units(d)}
        assert {c[3:8] for c in cases} == shapes
        for (Cn, H, K, k, s) in shapes:
            for op in R.OPS:
                assert ("f32", "default", op) in {c[:3] for c in cases if c[3:8] == (Cn, H, K, k, s)}
                assert ("bf16", R.bf16_route(L, op, N, Cn, H, K, k, s), op) in {c[:3] for c in cases if c[3:8] == (Cn, H, K, k, s)}
        for c in cases:
            if c[0] == "bf16":
                assert R.conv_plan(L, 1, c[1], c[2], N, *c[3:8]) is not None, (net, c)
        cl = R.trainer_conv_bn_cl_cases(L, d, N)
        assert cl == [layer for layer in R.trainer_layers(d) if layer[3] == 3], (net, cl)
        if net != "r50":
            assert {layer[1] // layer[4] for layer in cl} == {8, 4}, (net, cl)
        _kinds(L, cases, N)   # (a bf16 route the trainer takes plans the shape)


def test_layer_routes_answers_without_a_device():
    """mi_layer_routes (the planner the trainer and the operators run through; host only): an unknown dtype, policy or site is refused with
    -2 and an all-zero answer; every fp32 layer of ResNet-50 answers (MI_FWD_F32, MI_DG_F32, MI_WG_F32); the fp32 fz follows the site mask of
    RESNET_MI_F32_BNFUSE_BWD (default 4: the reductions above an identity block) and is 0 under the FULL policy; the stems take the matrix
    cores in both storage types"""
    import ctypes
    import os
    import synth
    from resnet_amd import binding as B
    L = _lib()
    out = (ctypes.c_int * 4)(9, 9, 9, 9)
    for bad in ((2, 0, 0), (-1, 0, 0), (0, 3, 0), (0, -1, 0), (0, 0, 3), (0, 0, 8)):
        assert L.mi_layer_routes(bad[0], bad[1], 8, 64, 56, 64, 1, 1, bad[2], out) == -2 and list(out) == [0, 0, 0, 0], bad
    assert R.layer_routes(L, 1, 0, 8, 48, 8, 80, 3, 1) is None      # no bf16 kernel tiles 48 -> 80 channels
    mask = int(os.environ.get("RESNET_MI_F32_BNFUSE_BWD", "4"))
    units = R.trainer_units(synth.R50_DIMS)
    assert {u[3] for u in units} == {0, 1, 2, 4}
    for _, role, shape, site in units:
        for policy in (B.MI_STORE_FAST, B.MI_STORE_RECOMPUTE_BN, B.MI_STORE_FULL):
            want_fz = int(bool(site & mask)) if policy != B.MI_STORE_FULL else 0
            assert R.layer_routes(L, 0, policy, R.N256, *shape, site=site) == (B.MI_FWD_F32, B.MI_DG_F32, B.MI_WG_F32, want_fz), (role, shape, site, policy)
    assert R.layer_routes(L, 0, 0, R.N256, *R.STEM) == (B.MI_FWD_STEM_F32, B.MI_DG_F32, B.MI_WG_STEM_F32, 0)
    assert R.layer_routes(L, 1, 0, R.N256, *R.STEM) == (B.MI_FWD_STEM_BF16, B.MI_DG_F32, B.MI_WG_STEM_BF16, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# mutants at N = 33: the partial last column tile
N33 = 33
TAIL_SHAPES = [(512, 7, 2048, 1, 1), (128, 28, 128, 3, 1)]


def _data33(shape):
    Cn, H, K, k, s = shape
    rng = np.random.default_rng(Cn + H + K + k)
    x = rng.standard_normal((N33, Cn, H, H), dtype=np.float32)
    w = (rng.standard_normal((K, Cn, k, k), dtype=np.float32) * np.float32((2.0 / (k * k * (Cn + K))) ** 0.5))
    return x, w


def _tail(L, shape):
    """the fp32 forward's plan at N = 33 and the columns [c0, cols) of its partial last tile"""
    Cn, H, K, k, s = shape
    p = R.conv_plan(L, 0, "default", "fwd", N33, Cn, H, K, k, s)
    bn = p[1]
    cols = N33 * (H // s) ** 2
    assert cols % bn, "a partial last tile"
    return p, cols - cols % bn, cols


@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=["C%d_H%d_K%d_k%d_s%d" % s for s in TAIL_SHAPES])
def test_mutant_partial_tile_misses_a_reduction_slice(shape):
    """6: the columns of the partial last tile miss one 32-channel reduction slice (rows of one 64-row tile): the checker of
    test_gpu_ragged.py, on its slabs at N = 33, rejects it; the correct result passes"""
    Cn, H, K, k, s = shape
    L = _lib()
    x, w = _data33(shape)
    Ho = H // s
    P = Ho * Ho
    plan, c0, cols = _tail(L, shape)
    seed = 3
    slabs = R.fwd_slabs(x, w, s, R.slab_images(N33, plan, K, P, seed), R.slab_channels(K, seed))
    got = _f32("fwd", x, w, None, shape)
    R.check_slabs(got, slabs, False, "valid fwd at N = 33")
    mat = got.transpose(1, 0, 2, 3).reshape(K, N33 * P).copy()
    part = _f32("fwd", x[:, 32:64], w[:, 32:64], None, (32, H, K, k, s)).transpose(1, 0, 2, 3).reshape(K, N33 * P)
    r0 = 64
    mat[r0:r0 + 64, c0:cols] -= part[r0:r0 + 64, c0:cols]
    bad = np.ascontiguousarray(mat.reshape(K, N33, Ho, Ho).transpose(1, 0, 2, 3))
    assert R.violations(bad, slabs, False) > 0


def _stats_tiles_f32(y, bn, pad_zeros=False):
    """per-channel (mean, biased var) of y [N, K, P] the way the epilogue partials merge: per column tile of bn columns a float32 two-pass,
    tiles merged in float32 (Chan).  pad_zeros: the mutant that counts the partial tile's masked columns as zeros"""
    K = y.shape[1]
    mat = y.transpose(1, 0, 2, 3).reshape(K, -1)
    cols = mat.shape[1]
    n, mean, m2 = np.zeros(K, np.float32), np.zeros(K, np.float32), np.zeros(K, np.float32)
    for c in range(0, cols, bn):
        t = mat[:, c:c + bn]
        if pad_zeros and t.shape[1] < bn:
            t = np.concatenate([t, np.zeros((K, bn - t.shape[1]), np.float32)], 1)
        cnt = np.float32(t.shape[1])
        mu = t.sum(1, dtype=np.float32) / cnt
        d = t - mu[:, None]
        q = (d * d).sum(1, dtype=np.float32)
        tot = n + cnt
        dd = mu - mean
        fr = cnt / tot
        m2 = (m2 + q + dd * dd * n * fr).astype(np.float32)
        mean = (mean + dd * fr).astype(np.float32)
        n = tot
    return mean, (m2 / n).astype(np.float32)


@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=["C%d_H%d_K%d_k%d_s%d" % s for s in TAIL_SHAPES])
def test_mutant_statistics_count_masked_columns(shape):
    """7: BN statistics that count the partial last tile's masked columns as zeros fail the statistics check of the conv + BN cases at
    N = 33; statistics merged from float32 tile partials pass"""
    Cn, H, K, k, s = shape
    L = _lib()
    x, w = _data33(shape)
    plan, c0, cols = _tail(L, shape)
    Rk = R.slab_channels(K, 5)
    slab = R.fwd_slabs(x, w, s, [0], Rk)[1]
    y = _f32("fwd", x, w, None, shape)
    gm, gv = _stats_tiles_f32(y, plan[1])
    assert R.conv_stats_violations(gm[Rk], gv[Rk], slab.ref, slab.A)[0] == 0
    gm, gv = _stats_tiles_f32(y, plan[1], pad_zeros=True)
    assert R.conv_stats_violations(gm[Rk], gv[Rk], slab.ref, slab.A)[0] > 0
