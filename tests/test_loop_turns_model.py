"""The loop-turn entries of tests/mutants.py on the CPU (no GPU), as tests/test_ewref.py and tests/test_input_aa.py hold theirs: the
fault restated in a float32 model that walks the data the way the kernel does (which element is whose thread's, in which turn), run on
the KILLER'S OWN inputs (imported, not copied) through the checker the GPU test calls -- the faulty model must fail it and the model
without a fault must pass it.  An input change that disarms a killer fails here.  Beside them the reach of the new cases from the
launchers' formulas, and that the cases the suite had do not reach the branches that survived it."""
import numpy as np
import pytest

import convref as R
import ewref as E
import lossref
import optim_ref
import perelement as P
import rrcref
import synth

F = np.float32


@pytest.fixture(scope="module", autouse=True)
def _threads():
    R.set_threads(16)


# ---------------------------------------------------------------------------------------------------------------------------
# reach
def test_loop_turn_shapes_are_on_their_branches():
    r = {s: E.bn_reach(*s) for s in E.LOOP_TURN_SHAPES}
    for s in (("f32", 64, 66, 1), ("bf16", 64, 66, 1)):
        assert (r[s]["V"], r[s]["units"], r[s]["whole"], r[s]["remainder"], r[s]["nsplit"]) == (4, 1089, 1, 65, 1)
        assert E.bn_reach(*s, in_flight=2)["whole"] == 2
    for s in (("f32", 2048, 48, 2), ("bf16", 2048, 48, 4)):
        assert r[s]["units"] == 1152 and r[s]["whole"] == 1 and r[s]["crosses"] and r[s]["remainder"] == 128
    for s in (("f32", 2048, 7, 21), ("bf16", 2048, 7, 21)):
        assert (r[s]["V"], r[s]["units"], r[s]["whole"], r[s]["remainder"]) == (1, 1029, 1, 5)
    for s in (("f32", 64, 4, 33), ("bf16", 64, 4, 33)):
        assert r[s]["nsplit"] == 32 and -(-33 // 32) == 2


def test_the_nets_planes_do_not_reach_what_survived():
    """at the batches a killer may use (N = 4 for the small nets, 8 for ResNet-50) no batch-norm shape runs the V == 1 whole turn or more
    than 16 splits"""
    for dims, N in ((synth.C1S_DIMS, 4), (synth.R50_DIMS, 8)):
        for Cn, H, _, _ in E.bn_shapes(dims):
            for pair in ("f32", "bf16"):
                r = E.bn_reach(pair, Cn, H, N)
                assert r["nsplit"] <= 16
                assert not (r["V"] == 1 and r["whole"])
                assert (r["whole"] > 0) == (r["units"] > 768)      # (a thread takes a whole turn where idx + 768 < units: 56^2 and 112^2 planes)


# ---------------------------------------------------------------------------------------------------------------------------
# batch-norm statistics as bn_stats_kernel walks them: block = (channel, split); unit idx of the block's images is thread idx % 256's; a
# thread takes whole turns of four units while idx + 768 < total, then single units
def _merge(a, b):
    """wel_merge on arrays of (n, mean, m2)"""
    n = (a[0] + b[0]).astype(F)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = (b[1] - a[1]).astype(F)
        f = np.where(n == 0, F(0), b[0] / np.where(n == 0, F(1), n)).astype(F)
    mean = np.where(n == 0, F(0), a[1] + d * f).astype(F)
    m2 = np.where(n == 0, F(0), a[2] + b[2] + d * d * a[0] * f).astype(F)
    return n, mean, m2


def _tree(w):
    """a butterfly of merges over the last axis (a power of two) down to one"""
    while w[0].shape[-1] > 1:
        h = w[0].shape[-1] // 2
        w = _merge(tuple(a[..., :h] for a in w), tuple(a[..., h:] for a in w))
    return tuple(a[..., 0] for a in w)


def _batch(v):
    """(n, mean, m2) of the float32 values v [threads, k] about their own mean"""
    k = F(v.shape[1])
    bm = (v.sum(1, dtype=F) / k).astype(F)
    d = (v - bm[:, None]).astype(F)
    return np.full(v.shape[0], k, F), bm, d


def stats_model(xc, ns, V, fault=None):
    """mean, biased var of one channel xc [N, P] (float32 values) through bn_stats_kernel -> bn_finalize_kernel"""
    parts = []
    for sp in range(ns):
        units = xc[sp::ns].reshape(-1, V)
        total = units.shape[0]
        T = 256
        w = (np.zeros(T, F), np.zeros(T, F), np.zeros(T, F))
        t = np.arange(T)
        idx = t.copy()
        while True:
            act = idx + 3 * T < total
            if not act.any():
                break
            v = np.stack([units[np.minimum(idx + u * T, total - 1)] for u in range(4)], 1)      # [T, 4, V]
            n, bm, d = _batch(v.reshape(T, 4 * V))
            sq = (d * d).astype(F).reshape(T, 4, V)
            if fault == "turn_unit3" and V > 1:
                sq[:, 3] = 0
            if fault == "turn_scalar_d4" and V == 1:
                sq[:, 3] = 0
            b = (np.where(act, n, F(0)), bm, sq.sum((1, 2), dtype=F))
            w = tuple(np.where(act, m, o) for m, o in zip(_merge(w, b), w))
            idx = np.where(act, idx + 4 * T, idx)
        while True:
            act = idx < total
            if not act.any():
                break
            v = units[np.minimum(idx, total - 1)]
            for q in range(0, V, 4) if V > 1 else (0,):
                if V > 1:
                    n, bm, d = _batch(v[:, q:q + 4])
                    sq = (d * d).astype(F)
                    if fault == "rem_add4_d4":
                        sq[:, 3] = 0
                    b = (n, bm, sq.sum(1, dtype=F))
                else:
                    b = (np.ones(T, F), (F(0.5) * v[:, 0]).astype(F) if fault == "rem_add1_half" else v[:, 0], np.zeros(T, F))
                b = (np.where(act, b[0], F(0)), b[1], b[2])
                w = tuple(np.where(act, m, o) for m, o in zip(_merge(w, b), w))
            idx = np.where(act, idx + T, idx)
        waves = _tree(tuple(a.reshape(4, 64) for a in w))
        r = tuple(a[0:1] for a in waves)
        for i in range(1, 4):
            b = tuple(a[i:i + 1] for a in waves)
            if fault == "interwave_n0" and i == 3:
                b = (np.zeros(1, F), b[1], b[2])
            r = _merge(r, b)
        parts.append(r)
    lanes = tuple(np.zeros(64, F) for _ in range(3))
    for sp, r in enumerate(parts):
        for a, v in zip(lanes, r):
            a[sp] = v[0]
        if fault == "finalize_lane16" and sp >= 16:
            lanes[2][sp] = 0
    n, mean, m2 = _tree(lanes)
    return mean, F(m2 / n)


def _stats_check(case, N, fault, channels=3):
    """E.stats_violations, as perelement.bn_fwd calls it, on the first slab channels of the killer's own input"""
    pair, Cn, H, _ = case
    x_dt, a_dt = P.PAIRS[pair]
    x = P.bn_fwd_inputs(case, N)["x"]
    Rc = R.slab_channels(Cn, Cn * 7 + H + 11 * x_dt + 13 * a_dt)[:channels]
    ns, V = E.bn_nsplit(N, Cn), E.bn_vec(pair, H * H)
    got = [stats_model(x[:, c].reshape(N, H * H), ns, V, fault) for c in Rc]
    gm, gv = np.array([g[0] for g in got], F), np.array([g[1] for g in got], F)
    return E.stats_violations(gm, gv, x[:, Rc])[0]


STATS = [("turn_unit3", ("f32", 64, 112, ("relu",)), 8),      # the entry's killer, r50_N8-f32_C64_H112; the next two: test_bn_loop_turns
         ("turn_unit3", ("f32", 64, 66, ("relu",)), 1), ("turn_unit3", ("bf16", 64, 66, ("relu",)), 1),
         ("turn_scalar_d4", ("f32", 2048, 7, ("relu",)), 21), ("rem_add4_d4", ("f32", 64, 8, ("relu",)), 4),
         ("rem_add1_half", ("f32", 512, 7, ("relu",)), 8), ("interwave_n0", ("f32", 64, 56, ("relu",)), 8),
         ("finalize_lane16", ("f32", 64, 4, ("relu",)), 33)]


@pytest.mark.parametrize("fault,case,N", STATS, ids=["%s-%s_C%d_H%d_N%d" % (f, c[0], c[1], c[2], n) for f, c, n in STATS])
def test_bn_statistics_faults_fail_on_their_killers_inputs(fault, case, N):
    assert _stats_check(case, N, None) == 0
    assert _stats_check(case, N, fault) > 0


def test_the_interwave_fault_is_invisible_at_16_units():
    """c1s_N4-f32_C64_H8 has 16 units per block: the fourth wave holds nothing, the fault changes no bit -- why that entry's killer is a 56^2 plane"""
    case = ("f32", 64, 8, ("relu",))
    x = P.bn_fwd_inputs(case, 4)["x"]
    a, b = stats_model(x[:, 0].reshape(4, 64), 4, 4), stats_model(x[:, 0].reshape(4, 64), 4, 4, "interwave_n0")
    assert a[0] == b[0] and a[1] == b[1]


# ---------------------------------------------------------------------------------------------------------------------------
# batch-norm backward sums as bn_bwd_reduce_kernel walks them (U units in flight: 4, the external-mask modes 2), bn_bwd_finalize_kernel
def bwd_sums_model(xc, gc, mean, var, ns, V, U, fault=None):
    """(dbeta, dgamma) of one channel: xc, gc [N, P] float32 (gc: the gated gradient)"""
    sd = np.sqrt(F(var) + F(E.EPS)).astype(F)
    s1p, s2p = np.zeros(64, F), np.zeros(64, F)
    for sp in range(ns):
        xu, gu = xc[sp::ns].reshape(-1, V), gc[sp::ns].reshape(-1, V)
        total = xu.shape[0]
        xh = ((xu - F(mean)) / sd).astype(F)
        idx = np.arange(total)
        t = idx % 256
        k = idx // 256
        whole_turns = 0
        while whole_turns * U * 256 + (U - 1) * 256 < total:                       # thread 0's count; thread t's own below
            whole_turns += 1
        turn = k // U
        in_whole = (turn * U * 256 + t + (U - 1) * 256) < total
        in1 = np.ones((total, V), bool)
        in2 = np.ones((total, V), bool)
        if fault == "turn_last_unit_s2":
            in2[in_whole & (k % U == U - 1)] = False
        if fault == "rem_last_element_s1":
            in1[~in_whole, V - 1] = False
        s1p[sp] = np.where(in1, gu, F(0)).sum(dtype=F)
        s2p[sp] = np.where(in2, gu * xh, F(0)).astype(F).sum(dtype=F)
        if fault == "finalize_lane16_s2" and sp >= 16:
            s2p[sp] = 0
    return s1p.sum(dtype=F), s2p.sum(dtype=F)


def _bwd_sums_check(case, N, fault, channels=3):
    pair, Cn, H, mode = case
    inp = P.bn_bwd_inputs(case, N)
    x, dy, on = inp["x"], inp["dy"], inp["on"]
    g = dy if on is None else np.where(on, dy, F(0))
    Rc = R.slab_channels(Cn, Cn * 5 + H)[:channels]
    ns, V, U = E.bn_nsplit(N, Cn), E.bn_vec(pair, H * H), 2 if mode == 3 else 4
    got = [bwd_sums_model(x[:, c].reshape(N, -1), g[:, c].reshape(N, -1), inp["means"][c], inp["vars_"][c], ns, V, U, fault) for c in Rc]
    db, dg = np.array([a[0] for a in got], F), np.array([a[1] for a in got], F)
    sums = E.grad_sums(g[:, Rc], x[:, Rc], inp["means"][Rc], inp["vars_"][Rc], E.EPS)
    return E.sums_violations(db, dg, sums)[0]


BWD = [("turn_last_unit_s2", ("f32", 64, 112, 1), 8),             # the entry's killer, r50_N8-f32_C64_H112_mode1
       ("turn_last_unit_s2", ("f32", 64, 66, 0), 1), ("turn_last_unit_s2", ("bf16", 64, 66, 3), 1),
       ("rem_last_element_s1", ("f32", 256, 8, 0), 4), ("finalize_lane16_s2", ("f32", 64, 4, 0), 33)]


@pytest.mark.parametrize("fault,case,N", BWD, ids=["%s-%s_C%d_H%d_mode%d_N%d" % ((f,) + c + (n,)) for f, c, n in BWD])
def test_bn_backward_sum_faults_fail_on_their_killers_inputs(fault, case, N):
    assert _bwd_sums_check(case, N, None) == 0
    assert _bwd_sums_check(case, N, fault) > 0


@pytest.mark.parametrize("dt,Cn,K", [("f32", 256, 128), ("bf16", 64, 256)])
def test_missing_eps_in_the_merged_sums_needs_a_small_variance(dt, Cn, K):
    """bn_bwd_parts_merge_kernel's s2 / sqrt(var + eps) written without eps: inside the bound of dgamma on the tensors the fused-dgrad
    cases normalise (variance 2.25), outside it in every small-variance channel of test_dgrad_bn_bwd_small_variance's"""
    case = (dt, Cn, 8, K, 1, 1, "")
    for small, want in ((False, False), (True, True)):
        inp = P.dgrad_bn_bwd_inputs(case, 4, small_var=small)
        x, means, vars_ = inp["bn_x"], inp["means"], inp["vars_"]
        g = np.where(inp["mask"] > 0, P.normal(x.shape, 9), F(0))
        rdb, rdg, adb, adg = R.bn_grad_sums(g, x, means, vars_, inp["eps"])
        with np.errstate(divide="ignore", invalid="ignore"):
            dg = (g.astype(np.float64) * (x.astype(np.float64) - means[None, :, None, None])).sum((0, 2, 3)) / np.sqrt(vars_.astype(np.float64))
        out = ~(np.abs(dg - rdg) <= R.C_FACTOR * R.U24 * adg)
        assert out.any() == want and (not want or out[::P.SMALL_VAR_EVERY].all())
        assert not want or vars_[::P.SMALL_VAR_EVERY].max() < 10 * inp["eps"]      # (bf16 storage leaves two or three levels: 7e-7)


def test_gate_and_store_entries_have_elements_to_show_on_their_killers_inputs():
    """bn_bwd_apply_gate_y_ge: c1s_N4-f32_C64_H8_mode1 plants x == mean in the beta == 0 channels (y == 0 exactly, dy != 0), and dx with the
    gate y >= 0 leaves the bounds there.  bn_bwd_reduce_remainder_gated_ungated: mode 3's mask is 0 where dy is not, in c1s_N4-f32_C256_H8_mode3.
    relu_deriv_gate_ge: test_bn_add_relu_and_external_mask[256-8-4]'s activation is exactly 0 in first elements of float4s whose upstream is not"""
    case, N = ("f32", 64, 8, 1), 4
    inp = P.bn_bwd_inputs(case, N)
    x, gamma, beta, means, vars_, dy, on = (inp[k] for k in ("x", "gamma", "beta", "means", "vars_", "dy", "on"))
    y0 = (x == means[None, :, None, None]) & (beta == 0)[None, :, None, None]
    assert (y0 & ~on & (dy != 0)).sum() > 100
    g = np.where(on, dy, F(0))
    sums = E.grad_sums(g, x, means, vars_, E.EPS)
    seed = 64 * 5 + 8 + 17 + 3000
    slabs = E.bn_dx_slabs(g, x, gamma, means, vars_, E.EPS, sums, R.slab_images(N, seed=seed), R.slab_channels(64, seed))
    c = lambda v: v[None, :, None, None]
    sd = np.sqrt(vars_ + F(E.EPS)).astype(F)
    xh = ((x - c(means)) / c(sd)).astype(F)
    M = F(N * 64)
    for ge, want in ((False, False), (True, True)):
        gq = np.where(on | (ge & y0), dy, F(0))
        dx = (c(gamma / sd) * (gq - c((sums[0] / M).astype(F)) - xh * c((sums[1] / M).astype(F)))).astype(F)
        assert (R.violations(dx, slabs, False) > 0) == want
    inp = P.bn_bwd_inputs(("f32", 256, 8, 3), 4)
    assert ((inp["mask"] <= 0) & (inp["dy"] != 0)).sum() > 1000
    from util import nchw, rand
    xb, res = nchw(rand((4, 8, 8, 256), 13)), nchw(rand((4, 8, 8, 256), 14))          # the test's own operands, its gy in float64
    gam, bet = (1 + 0.2 * rand((256,), 15)).astype(F), (0.3 * rand((256,), 16)).astype(F)
    mu, var = E.stats_ref(xb)[:2]
    gy = E.apply_ref(xb, gam, bet, mu, var, 1e-7, False, res)[0].ravel()
    up = nchw(rand((4, 8, 8, 256), 17)).ravel()
    assert ((gy[::4] == 0) & (up[::4] != 0)).sum() > 1000


# ---------------------------------------------------------------------------------------------------------------------------
# the straddling vectors of 7 x 7 planes: element e of the flattened tensor belongs to channel (e / P) % C, its vector starts in channel
# ((e / V) V / P) % C; the faults give the spill elements one of the first channel's scalars
def _channels(shape, V):
    Nn, Cn, H, _ = shape
    e = np.arange(Nn * Cn * H * H)
    return (e // (H * H)) % Cn, ((e // V * V) // (H * H)) % Cn


def test_straddle_faults_fail_on_their_killers_inputs():
    # bn_apply_straddle_sd on r50_N8-f32_C512_H7
    case, N = ("f32", 512, 7, ("relu",)), 8
    inp = P.bn_fwd_inputs(case, N)
    x, gamma, beta = inp["x"], inp["gamma"], inp["beta"]
    means, vars_ = (a.astype(F) for a in E.stats_ref(x)[:2])
    seed = 512 * 7 + 7
    slabs = E.bn_apply_slabs(x, gamma, beta, means, vars_, E.EPS, True, None, R.slab_images(N, seed=seed), R.slab_channels(512, seed))
    c, cv = _channels(x.shape, 4)
    sd = np.sqrt(vars_ + F(E.EPS)).astype(F)
    for fault, want in ((False, False), (True, True)):
        y = np.maximum(gamma[c] * ((x.ravel() - means[c]) / sd[cv if fault else c]) + beta[c], F(0)).astype(F).reshape(x.shape)
        assert (R.violations(y, slabs, False) > 0) == want
    # bn_bwd_apply_straddle_k2 on r50_N8-f32_C2048_H7_mode0
    case = ("f32", 2048, 7, 0)
    inp = P.bn_bwd_inputs(case, N)
    x, gamma, means, vars_, g = inp["x"], inp["gamma"], inp["means"], inp["vars_"], inp["dy"]
    sums = E.grad_sums(g, x, means, vars_, E.EPS)
    seed = 2048 * 5 + 7 + 3000
    slabs = E.bn_dx_slabs(g, x, gamma, means, vars_, E.EPS, sums, R.slab_images(N, seed=seed), R.slab_channels(2048, seed))
    c, cv = _channels(x.shape, 4)
    sd = np.sqrt(vars_ + F(E.EPS)).astype(F)
    M = F(N * 49)
    k1, k2 = (sums[0] / M).astype(F), (sums[1] / M).astype(F)
    xh = ((x.ravel() - means[c]) / sd[c]).astype(F)
    for fault, want in ((False, False), (True, True)):
        dx = ((gamma / sd)[c] * (g.ravel() - k1[c] - xh * k2[cv if fault else c])).astype(F).reshape(x.shape)
        assert (R.violations(dx, slabs, False) > 0) == want


# ---------------------------------------------------------------------------------------------------------------------------
# max-pool: the tap entries of the 3x3 / stride-2 kernels on the ragged case's input, the generic kernels on test_gpu_ops.py::test_maxpool's
def _maxpool_fwd_skipping(x, skip):
    """ewref.maxpool_fwd_ref with the taps skip(r, c, ow) (a bool per output column) never winning"""
    N, Cn, H, _ = x.shape
    Ho = H // 2
    xp = np.full((N, Cn, H + 2, H + 2), -np.inf, F)
    xp[:, :, 1:H + 1, 1:H + 1] = x
    mv = np.full((N, Cn, Ho, Ho), -1024.0, F)
    mi = np.full((N, Cn, Ho, Ho), -1024, np.int32)
    base = (np.arange(N * Cn, dtype=np.int32) * np.int32(H * H)).reshape(N, Cn, 1, 1)
    o = np.arange(Ho, dtype=np.int32)
    for r in (-1, 0, 1):
        for c in (-1, 0, 1):
            cand = xp[:, :, r + 1:r + 1 + 2 * Ho:2, c + 1:c + 1 + 2 * Ho:2]
            upd = (cand > mv) & ~skip(r, c, o)[None, None, None, :]
            mv = np.where(upd, cand, mv)
            mi = np.where(upd, base + ((2 * o[:, None] + r) * H + 2 * o[None, :] + c), mi)
    return mv, mi


def test_maxpool_tap_faults_fail_on_the_ragged_input():
    d = synth.C1S_DIMS
    H = d["input"] // d["init_conv_stride"]
    inp = P.maxpool_inputs(P.F32, 4, d["init_conv_filters"], H)
    x, dy = inp["x"], inp["dy"]
    y, idx = E.maxpool_fwd_ref(x)
    none = _maxpool_fwd_skipping(x, lambda r, c, o: np.zeros(o.shape, bool))
    assert np.array_equal(none[0], y) and np.array_equal(none[1], idx)
    left = _maxpool_fwd_skipping(x, lambda r, c, o: (c == -1) & (o % 4 == 0) & (o > 0))
    last = _maxpool_fwd_skipping(x, lambda r, c, o: (r == 1) & (c == 1) & (o % 4 == 3))
    assert not np.array_equal(left[1], idx) and not np.array_equal(last[1], idx)
    # maxpool_bwd_v11_first_writer: element (2a + 1, 2b + 1) named by window (a, b) and by (a + 1, b + 1) takes the first one's dy
    Ho = H // 2
    ref = E.maxpool_bwd_ref(idx, dy, H)
    bad = ref.copy().reshape(-1)
    both = idx[:, :, :-1, :-1] == idx[:, :, 1:, 1:]
    e11 = (2 * np.arange(Ho - 1)[:, None] + 1) * H + 2 * np.arange(Ho - 1)[None, :] + 1
    both &= (idx[:, :, :-1, :-1] % (H * H)) == e11[None, None]
    bad[idx[:, :, :-1, :-1][both]] = dy[:, :, :-1, :-1][both]
    assert both.any() and not np.array_equal(bad.reshape(ref.shape), ref)


def _maxpool_generic(x, ge=False):
    """maxpool_fwd_kernel (k = 3, stride 2) on any plane, by windows: values, flat NCHW indices; ge: the last of equal maxima"""
    N, Cn, H, _ = x.shape
    Ho = H // 2
    mv = np.full((N, Cn, Ho, Ho), -1024.0, F)
    mi = np.full((N, Cn, Ho, Ho), -1024, np.int64)
    base = (np.arange(N * Cn) * H * H).reshape(N, Cn)
    for oh in range(Ho):
        for ow in range(Ho):
            for r in (-1, 0, 1):
                for c in (-1, 0, 1):
                    ih, iw = 2 * oh + r, 2 * ow + c
                    if 0 <= ih < H and 0 <= iw < H:
                        v = x[:, :, ih, iw]
                        upd = v >= mv[:, :, oh, ow] if ge else v > mv[:, :, oh, ow]
                        mv[:, :, oh, ow] = np.where(upd, v, mv[:, :, oh, ow])
                        mi[:, :, oh, ow] = np.where(upd, base + ih * H + iw, mi[:, :, oh, ow])
    return mv, mi


def test_generic_maxpool_faults_fail_on_the_operator_tests_inputs():
    from util import nchw, rand
    x = nchw(np.maximum(rand((3, 12, 12, 64), 21), 0))
    assert not np.array_equal(_maxpool_generic(x, ge=True)[1], _maxpool_generic(x)[1])          # test_maxpool[64-12-3]: ties at 0
    x = nchw(np.maximum(rand((3, 13, 13, 64), 21), 0))                                           # test_maxpool[64-13-3]
    idx = _maxpool_generic(x)[1]
    dy = nchw(rand((3, 6, 6, 64), 22))
    lastw, firstw = np.zeros(x.size, F), np.zeros(x.size, F)
    for oh in range(6):
        for ow in range(6):
            lastw[idx[:, :, oh, ow]] = dy[:, :, oh, ow]
    for oh in reversed(range(6)):
        for ow in reversed(range(6)):
            firstw[idx[:, :, oh, ow]] = dy[:, :, oh, ow]
    assert not np.array_equal(lastw, firstw)


# ---------------------------------------------------------------------------------------------------------------------------
# soft-max, loss head, average pool, Adam
def _softmax_f32_max_of(x, cols, scale_from=None):
    """E.softmax_f32 with the maximum over the first `cols` columns; scale_from: the sum's terms from that column on scaled by 1 + 2^-10"""
    x = x.astype(F)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(x - x[:, :cols].max(1, keepdims=True))
        t = e.copy()
        if scale_from is not None:
            t[:, scale_from:] *= F(1.0009765625)
        return (e / t.sum(1, keepdims=True, dtype=F)).astype(F)


@pytest.mark.parametrize("L", E.DOMINANT_L)
def test_softmax_maximum_of_the_first_turn_fails_on_dominant_rows(L):
    x = E.dominant_rows(L)
    ref, A = E.softmax_ref(x)
    assert R.dist_f32(E.softmax_f32(x), ref, A)[1] == 0
    assert R.dist_f32(_softmax_f32_max_of(x, 64), ref, A)[1] > 0
    cols = E.dominant_columns(L)
    assert all(c >= 64 for c in cols[:-1]) and cols[-1] == -1 and (L <= 960 or any(960 <= c < 1024 for c in cols))
    for r, c in enumerate(cols[:-1]):
        assert x[r, c] - np.delete(x[r], c).max() > 89


def test_softmax_maximum_of_the_first_turn_passed_the_rows_the_suite_had():
    """the survivor: on softmax_rows (the ragged and batch-256 inputs) the same fault stays inside the bound"""
    x = P.softmax_ce_inputs(8, 1000)["x"]
    ref, A = E.softmax_ref(x)
    assert R.dist_f32(_softmax_f32_max_of(x, 64), ref, A)[1] == 0
    assert R.dist_f32(_softmax_f32_max_of(x, 1000, scale_from=64), ref, A)[1] > 0    # the scaled second turn of the sum does fail there


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("L", E.DOMINANT_L)
def test_loss_head_maximum_of_the_first_turn_fails_on_dominant_rows(L, eps):
    x, lab = lossref.dominant_inputs(L)
    assert all(0 <= c < L for c in lab) and (lab > 63).any()
    ref = lossref.loss_head(x, lab, eps)[2]
    ok = lossref.loss_head_f32(x, lab, eps)
    assert np.all(np.abs(ok.astype(np.float64) - ref) <= lossref.loss_bound(ref))
    bad = lossref.loss_head_f32_max_of(x, lab, eps, 64)
    assert not np.all(np.isfinite(bad)) or not np.all(np.abs(bad.astype(np.float64) - ref) <= lossref.loss_bound(ref))


@pytest.mark.parametrize("shape", [(8, 1000), (7, 1537)])
def test_loss_head_maximum_of_the_first_turn_changes_the_bits_of_pred(shape):
    """how test_loss_head[shape4-0.1] / [shape5-0.1] kill the two maximum entries: pred must have the soft-max operator's bits, and on
    make_inputs the maximum of the first 64 columns is another number in most rows, so exp(x - mx) / s is rounded elsewhere"""
    x, _ = lossref.make_inputs(*shape)
    assert (x[:, :64].max(1) != x.max(1)).sum() >= shape[0] // 2
    assert np.count_nonzero(_softmax_f32_max_of(x, 64).view(np.uint32) != E.softmax_f32(x).view(np.uint32)) > 100


def test_loss_rank_without_the_last_slot_differs_on_the_workloads_row():
    x, lab = lossref.make_inputs(8, 1000)
    pred = lossref.softmax(x).astype(F)
    full = lossref.rank_of(pred, lab)
    cut = pred.copy()
    cut[:, 960:] = -1          # columns 960 .. 999 never count
    for r in range(8):
        if lab[r] >= 960:
            cut[r, lab[r]] = pred[r, lab[r]]
    assert not np.array_equal(lossref.rank_of(cut, lab), full)


@pytest.mark.parametrize("dt", [P.F32, P.BF16])
def test_avgpool_without_the_second_lane_turn_fails(dt):
    x = P.avgpool_inputs(dt, 2, 64, 9)["x"].reshape(2, 64, 81)
    ref, A = E.avgpool_ref(x.reshape(2, 64, 9, 9))
    assert R.dist_f32(x.sum(2, dtype=F) / F(81), ref, A)[1] == 0
    assert R.dist_f32(x[..., :64].sum(2, dtype=F) / F(81), ref, A)[1] > 0
    old = P.avgpool_inputs(dt, 8, 2048, 7)["x"]
    assert old.shape[2] * old.shape[3] <= 64     # the planes the suite had: one turn


def test_adam_second_turn_faults_fail():
    (p, g, m, v), bad_g, hp = E.adam_second_turn_inputs()
    first = E.ADAM_GRID_CAP * 256
    assert p.size - first == 257 and (bad_g < first).any() and (bad_g >= first).any()
    tail = tuple(a[first:] for a in (p, g, m, v))
    got = E.adam_f32(*tail, **hp)
    assert E.adam_violations(got, tail, hp)[0] == 0
    swapped = E.adam_f32(*tail, **dict(hp, cb2=hp["cb1"]))
    assert E.adam_violations(swapped, tail, hp)[0] > 0
    nodecay = E.adam_f32(*tail, **hp)[0] + F(hp["wd"]) * tail[0]
    assert E.adam_violations((nodecay, got[1], got[2]), tail, hp)[0] > 0


def test_adam_without_decoupled_decay_fails_the_operator_tests_norm():
    """test_gpu_ops.py::test_softmax_ce_adam: rel-L2 of p against the oracle below 1e-6"""
    from util import rand, rel_l2
    n = 10007
    p, g = rand((n,), 61), rand((n,), 62, 0.01)
    m, v = rand((n,), 63, 0.001), np.abs(rand((n,), 64, 1e-4))
    hp = dict(lr=1e-4, wd=1e-3, b1=0.9, b2=0.999, cb1=0.9 ** 3, cb2=0.999 ** 3, eps=1e-7)
    good = E.adam_f32(p, g, m, v, **hp)[0]
    ref = E.adam_ref(p, g, m, v, **hp)[0][0]
    assert rel_l2(good, ref) < 1e-6
    assert rel_l2(good + F(hp["wd"]) * p, ref) > 1e-6


# ---------------------------------------------------------------------------------------------------------------------------
# LARS / SGD
def _optim_case(offs, seed):
    from test_gpu_optim import _spread_state
    return _spread_state(offs, seed)


def _update_fails(kind, offs, is_w, w, g, b, lr, wd, fault):
    from test_gpu_optim import MU, NORM_REL, TAU, _check_update, _split
    ws, gs, bs = _split(w, offs), _split(g, offs), _split(b, offs)
    ref_w, _, ref_b, _ = optim_ref.step(kind, ws, gs, bs, is_w, float(F(lr)), wd, MU, TAU)
    bad_w, _, bad_b, _ = optim_ref.step(kind, ws, gs, bs, is_w, float(F(lr)), wd, MU, TAU, fault=fault)
    ref_sq = optim_ref.sq_norms(ws, gs)
    sq = np.array([[np.sum(np.square(wi.astype(np.float64)[~mk[0]])), np.sum(np.square(gi.astype(np.float64)[~mk[1]]))]
                   for wi, gi, mk in ((wi, gi, optim_ref._fault_masks(wi.size, fault)) for wi, gi in zip(ws, gs))])
    if kind == optim_ref.LARS and (np.abs(sq - ref_sq) / np.maximum(ref_sq, 1e-300)).max() > NORM_REL:
        return True
    try:
        _check_update(fault, [a.astype(F) for a in bad_w], [a.astype(F) for a in bad_b], ref_w, ref_b)
    except AssertionError:
        return True
    return False


SCALAR_TAIL = [0, 64, 64 + 4096, 64 + 4096 + 8192 + 7]   # test_operator_scalar_tail's tensors


@pytest.mark.parametrize("kind,fault", [(optim_ref.LARS, "norm_whole_last_quad"), (optim_ref.LARS, "norm_partial_second_turn"),
                                        (optim_ref.LARS, "norm_wave3"), (optim_ref.SGD, "update_partial_second_turn_no_momentum"),
                                        (optim_ref.SGD, "update_whole_last_w_no_decay")])
def test_optimizer_faults_fail_on_the_scalar_tail_tensors(kind, fault):
    w, g, b = _optim_case(SCALAR_TAIL, 41)
    lr = 0.5 if kind == optim_ref.LARS else 0.01
    assert not _update_fails(kind, SCALAR_TAIL, [0, 1, 1], w, g, b, lr, float(F(5e-5)), None)
    assert _update_fails(kind, SCALAR_TAIL, [0, 1, 1], w, g, b, lr, float(F(5e-5)), fault)


@pytest.mark.parametrize("fault", ["guard_gn_only", "trust_second_lane_turn"])
def test_lars_faults_fail_on_the_loop_turn_tensors(fault):
    offs, is_w = optim_ref.LOOP_TURN_OFFSETS, optim_ref.LOOP_TURN_IS_WEIGHT
    assert [len(optim_ref.chunks_of(s)) for s in optim_ref.LOOP_TURN_SIZES] == [1, 1, 66, 1]
    assert optim_ref.chunks_of(optim_ref.LOOP_TURN_SIZES[3])[0] // 4 == 2 * 256 + 1 and all(o % 4 == 0 for o in offs[:-1])
    w, g, b = _optim_case(offs, 51)
    w[offs[1]:offs[2]] = 0
    b[offs[1]:offs[2]] = 0
    assert not _update_fails(optim_ref.LARS, offs, is_w, w, g, b, 0.5, float(F(5e-5)), None)
    assert _update_fails(optim_ref.LARS, offs, is_w, w, g, b, 0.5, float(F(5e-5)), fault)


# ---------------------------------------------------------------------------------------------------------------------------
# the plain resample: the column table's second turn and the staging's second lane turn
def _resample_faulty(src, boxes, D, fault):
    """rrcref.resample with one planted fault of resample_u8_kernel: "ctab": the horizontal weight of output columns 256 and up is 0;
    "stage": the bytes of a source row from 1024 on, counted from its span's first byte rounded down to 16, are 0"""
    n, dim_in = src.shape[0], src.shape[1]
    out = np.empty((n, 3, D, D), F)
    import augref
    for i in range(n):
        r0, c0, h, w, fl = rrcref.clamp_box(boxes[i], dim_in)
        b = src[i, r0:r0 + h, c0:c0 + w, :].astype(np.int64).reshape(h, w * 3)
        if fault == "stage":
            for y in range(h):
                g = ((i * dim_in + r0 + y) * dim_in + c0) * 3
                b[y, max(0, 1024 - (g & 15)):] = 0
        b = b.reshape(h, w, 3)
        y0, y1, wy = rrcref.coords(h, D)
        x0, x1, wx = rrcref.coords(w, D, fl)
        if fault == "ctab":
            wx = np.where(np.arange(D) >= 256, 0, wx)
        wy, wx = wy[:, None, None], wx[None, :, None]
        top = b[y0][:, x0] * (256 - wx) + b[y0][:, x1] * wx
        bot = b[y1][:, x0] * (256 - wx) + b[y1][:, x1] * wx
        v = top * (256 - wy) + bot * wy
        for d in range(3):
            out[i, d] = (v[:, :, 2 - d].astype(np.float64) * 2.0 ** -16 - augref.MEAN_OF_SRC[2 - d]).astype(F)
    return out


def test_resample_later_turn_faults_change_the_wide_case_and_nothing_the_suite_had():
    from test_gpu_input_rrc import WIDE_IN, WIDE_OUT, sweep_boxes, wide_boxes
    rng = np.random.RandomState(344260)
    boxes = wide_boxes()
    src = rng.randint(0, 256, size=(len(boxes), WIDE_IN, WIDE_IN, 3), dtype=np.uint8)
    ref = rrcref.resample(src, boxes, WIDE_OUT)
    assert np.array_equal(_resample_faulty(src, boxes, WIDE_OUT, None), ref)
    for fault in ("ctab", "stage"):
        changed = (_resample_faulty(src, boxes, WIDE_OUT, fault) != ref).reshape(len(boxes), -1).sum(1)
        assert changed[:3].all() and (fault == "ctab" or changed[3] == 0), (fault, changed)
    assert WIDE_OUT > 256 and (3 * 340 + 30) // 16 > 64
    # the widest case the suite had: 257 -> 224, 33 boxes
    rng = np.random.RandomState(257 * 1000 + 224 + 33)
    src = rng.randint(0, 256, size=(33, 257, 257, 3), dtype=np.uint8)
    boxes = sweep_boxes(33, 257, 224, rng)
    ref = rrcref.resample(src, boxes, 224)
    for fault in ("ctab", "stage"):
        assert np.array_equal(_resample_faulty(src, boxes, 224, fault), ref)


def _decode_stage_fault(src, pl, D, fault):
    """augref.decode with decode_stage_second_turn_zero restated: workgroups of 16 output rows stage CH = (3 D + 30) / 16 pieces per row,
    item r CH + c is thread (r CH + c) % 256's; the pieces of items 256 and up are zeros -- the bytes of row r's span from
    16 max(0, 256 - r CH) on, counted from the span's first byte rounded down to 16"""
    import augref
    t = augref.table()
    n, dim_in = src.shape[0], src.shape[1]
    CH = (3 * D + 30) // 16
    out = np.empty((n, 3, D, D), F)
    for i in range(n):
        ro, co, fl = (int(v) for v in pl[i])
        crop = src[i, ro:ro + D, co:co + D, :].reshape(D, 3 * D).copy()
        for h in range(D if fault else 0):
            c_min = max(0, 256 - (h % 16) * CH)
            if c_min < CH:
                g = ((i * dim_in + ro + h) * dim_in + co) * 3
                crop[h, max(0, 16 * c_min - (g & 15)):] = 0
        crop = crop.reshape(D, D, 3)
        if fl:
            crop = crop[:, ::-1, :]
        for d in range(3):
            out[i, d] = t[2 - d][crop[:, :, 2 - d]]
    return out


def test_decode_staging_fault_changes_the_killers_image():
    import augref
    from test_gpu_input_u8 import sweep_plan
    rng = np.random.RandomState(256 * 1000 + 224 + 1)                    # test_decode_sweep[256-224-1]
    src = rng.randint(0, 256, size=(1, 256, 256, 3), dtype=np.uint8)
    pl = sweep_plan(1, 32, rng)
    ref = augref.decode(src, pl, 224)
    assert np.array_equal(_decode_stage_fault(src, pl, 224, False), ref)
    assert np.count_nonzero(_decode_stage_fault(src, pl, 224, True) != ref) > 10000
    rng = np.random.RandomState(37 * 1000 + 30 + 33)                     # 37 -> 30: 16 x 7 pieces, one turn
    src = rng.randint(0, 256, size=(33, 37, 37, 3), dtype=np.uint8)
    pl = sweep_plan(33, 7, rng)
    assert np.array_equal(_decode_stage_fault(src, pl, 30, True), augref.decode(src, pl, 30))


def test_decode_and_resample_killers_take_the_later_turns():
    """host arithmetic of the launchers: 256 -> 224 takes a second staging turn and a second quad turn in both kernels; 40 -> 33 takes the
    element-wise quad stores (dim_out % 4 != 0) with at least one quad per row"""
    D = 224
    ch = (D * 3 + 30) // 16
    assert 16 * ch > 256 and 16 * (D // 4) > 256
    assert rrcref.launch_rows(256, D) * (D // 4) > 256
    assert 33 % 4 != 0 and 33 // 4 >= 1
