"""The per-element checks of test_gpu_batch256.py and test_gpu_batch256_ew.py at batches whose column counts end in a partial tile.

Every ResNet-50 plane has 2^j * 49 pixels, so at N = 256 every layer's N * P columns fill whole tiles on every route.  At N = 33 every fwd /
dgrad plan of ResNet-50 ends in a partial last column tile (a few of them inside a sliced tail round), and the list still reaches every plan
kind of the batch-256 list (test_convref.py).  The trajectory tests' nets run at their own batches: C1S and C4I at N = 4 (8 x 8 and 4 x 4
planes: a 4 x 4 forward is one 128-column tile holding 64 columns) and ResNet-50 at N = 8, with their stems at 32^2 and 224^2.

Per net: every (layer, route) pair of convref.trainer_conv_cases; conv + BN on the NCHW, channel-last and stem routes (every one fuses its
statistics); dgrad + BN' at the fusion sites; every batch-norm site in every form and mode (ewref.trainer_bn_*_cases); both stems forward
and weight gradient, in bf16 mode with the bf16 output and the bf16 dY; max-pool, average pool, soft-max with ce_deriv, the three FC GEMM
forms and the NHWC -> NCHW conversion.  Bounds and checkers are the batch-256 files' (tests/perelement.py).
"""
import os
import resource
import time

import pytest

import convref as R
import ewref as E
import perelement as P

pytestmark = pytest.mark.gpu

RUNS = [("r50", 33), ("c1s", 4), ("c4i", 4), ("r50", 8)]   # (net, N)
WORST = {}  # ("net N", kernel / dtype, route, op) -> worst distance, printed at the end of the module


def _recorder(net, N):
    tag = "%s N=%d" % (net, N)

    def record(key, worst):
        k = (tag,) + tuple(key)
        WORST[k] = max(WORST.get(k, 0.0), worst)
    return record


try:
    from resnet_amd import binding as _B
    _L = _B.load()
except RuntimeError:  # library not built: collection must still work; the tests then fail in the ops fixture
    _L = None
DIMS = R.nets()


def _runs(build):
    """[(net, N, item)] over RUNS and ids "net_N<N>-<item id>" """
    out, ids = [], []
    for net, N in RUNS:
        for item, iid in build(DIMS[net], N):
            out.append((net, N, item))
            ids.append("%s_N%d-%s" % (net, N, iid))
    return out, ids


def _last_plane(d):
    b = R.blocks(d)[-1]
    return b["H"] // b["s"]


CONV, CONV_IDS = _runs(lambda d, N: [(c, "%s_%s_%s_C%d_H%d_K%d_k%d_s%d" % c[:8]) for c in (R.trainer_conv_cases(_L, d, N) if _L else [])])
CONV_BN, CONV_BN_IDS = _runs(lambda d, N: [((c, "default"), "%s_C%d_H%d_K%d_k%d_s%d" % c[:6]) for c in R.trainer_conv_bn_cases(d)]
                             + [((("bf16",) + c, "cl"), "bf16_cl_C%d_H%d_K%d_k%d_s%d" % c[:5]) for c in (R.trainer_conv_bn_cl_cases(_L, d, N) if _L else [])])
DGRAD_BN, DGRAD_BN_IDS = _runs(lambda d, N: [(c, "%s_C%d_H%d_K%d_k%d_s%d" % c[:6]) for c in (R.trainer_dgrad_bn_cases(_L, d, N) if _L else [])])
STEM, STEM_IDS = _runs(lambda d, N: [((dt, op, dy), "%s_%s%s" % (dt, op, "_bf16dy" if dy == P.BF16 else ""))
                                     for dt, op, dy in (("f32", "fwd", P.F32), ("bf16", "fwd", P.F32), ("f32", "wgrad", P.F32),
                                                        ("bf16", "wgrad", P.F32), ("bf16", "wgrad", P.BF16))])
STEM_BN, STEM_BN_IDS = _runs(lambda d, N: [(v, v.replace(" ", "_")) for v in P.STEM_BN])
BN_FWD, BN_FWD_IDS = _runs(lambda d, N: [(c, "%s_C%d_H%d" % c[:3]) for c in E.trainer_bn_fwd_cases(d)])
BN_BWD, BN_BWD_IDS = _runs(lambda d, N: [(c, "%s_C%d_H%d_mode%d" % c) for c in E.trainer_bn_bwd_cases(d)])
EW, EW_IDS = _runs(lambda d, N: [(("maxpool", dt), "maxpool_%s" % n) for dt, n in ((P.F32, "f32"), (P.BF16, "bf16"))]
                   + [(("avgpool", dt), "avgpool_%s" % n) for dt, n in ((P.F32, "f32"), (P.BF16, "bf16"))]
                   + [(("fc", f), "fc_%s" % f) for f in ("nn", "lt", "rt")]
                   + [(("softmax", None), "softmax_ce_deriv"), (("nhwc", None), "nhwc_to_nchw")])


@pytest.fixture(scope="module", autouse=True)
def _threads():
    R.set_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))
    t0 = time.time()
    yield
    print("\nworst distance per net, route and op (fp32 and reductions: x 2^-24 A or sum|terms|, bf16: bf16 ulps); module %.0f s, peak host RSS "
          "%.2f GB" % (time.time() - t0, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20))
    for key in sorted(WORST, key=str):
        print("  %-10s %s  %.3g" % (key[0], " / ".join(str(k) for k in key[1:]), WORST[key]))


@pytest.mark.parametrize("run", CONV, ids=CONV_IDS)
def test_conv_route_ragged(ops, run):
    net, N, case = run
    P.conv_route(ops, case, N, _recorder(net, N))


@pytest.mark.parametrize("run", CONV_BN, ids=CONV_BN_IDS)
def test_conv_bn_fwd_ragged(ops, run):
    net, N, (case, route) = run
    P.conv_bn_fwd(ops, case, N, _recorder(net, N), route=route)


@pytest.mark.parametrize("run", DGRAD_BN, ids=DGRAD_BN_IDS)
def test_dgrad_bn_bwd_ragged(ops, run):
    net, N, case = run
    P.dgrad_bn_bwd(ops, case, N, _recorder(net, N))


@pytest.mark.parametrize("run", STEM, ids=STEM_IDS)
def test_stem_ragged(ops, run):
    net, N, (dt, op, dy_dt) = run
    P.stem(ops, dt, op, N, DIMS[net]["input"], _recorder(net, N), dy_dt=dy_dt)


@pytest.mark.parametrize("run", STEM_BN, ids=STEM_BN_IDS)
def test_stem_bn_fwd_ragged(ops, run):
    net, N, variant = run
    P.stem_bn_fwd(ops, variant, N, DIMS[net]["input"], _recorder(net, N))


@pytest.mark.parametrize("run", BN_FWD, ids=BN_FWD_IDS)
def test_bn_fwd_ragged(ops, run):
    net, N, case = run
    P.bn_fwd(ops, case, N, _recorder(net, N))


@pytest.mark.parametrize("run", BN_BWD, ids=BN_BWD_IDS)
def test_bn_bwd_ragged(ops, run):
    net, N, case = run
    P.bn_bwd(ops, case, N, _recorder(net, N))


# The loop turns of the batch-norm reductions that no plane of the three nets takes at N <= 8 (ewref.LOOP_TURN_SHAPES says which
# shape takes which turn; tests/test_loop_turns_model.py holds the reach from the launchers' formulas without a GPU).  Checkers, references
# and bounds are those of the lists above.
LT_FWD = [((pair, Cn, H, ("relu",)), N) for pair, Cn, H, N in E.LOOP_TURN_SHAPES]
LT_BWD = [((pair, Cn, H, mode), N) for pair, Cn, H, N in E.LOOP_TURN_SHAPES for mode in E.MODE_ORDER]


@pytest.mark.parametrize("run", LT_FWD, ids=["%s_C%d_H%d_N%d" % (c[0], c[1], c[2], n) for c, n in LT_FWD])
def test_bn_loop_turns(ops, run):
    case, N = run
    P.bn_fwd(ops, case, N, _recorder("turns", N))


@pytest.mark.parametrize("run", LT_BWD, ids=["%s_C%d_H%d_N%d_mode%d" % (c[0], c[1], c[2], n, c[3]) for c, n in LT_BWD])
def test_bn_bwd_loop_turns(ops, run):
    case, N = run
    P.bn_bwd(ops, case, N, _recorder("turns", N))


SMALL_VAR = {"f32": ("c4i_N4", "f32_C256_H8_K128_k1_s1"), "bf16": ("c1s_N4", "bf16_C64_H8_K256_k1_s1")}


@pytest.mark.parametrize("dt", list(SMALL_VAR))
def test_dgrad_bn_bwd_small_variance(ops, dt):
    """the fused dgrad + BN' cases normalise tensors of variance 2.25, where eps = 1e-7 cannot be seen; here every 8th channel has a
    variance of the size of eps (perelement.dgrad_bn_bwd_inputs, small_var), so that bn_bwd_parts_merge_kernel's s2 / sqrt(var + eps)
    is held to it"""
    run = [r for r, i in zip(DGRAD_BN, DGRAD_BN_IDS) if i == "%s-%s" % SMALL_VAR[dt]]
    assert len(run) == 1, "the case list no longer holds %s-%s" % SMALL_VAR[dt]
    net, N, case = run[0]
    P.dgrad_bn_bwd(ops, case, N, _recorder(net + " small var", N), small_var=True)


@pytest.mark.parametrize("dt", [P.F32, P.BF16], ids=["f32", "bf16"])
def test_avgpool_second_lane_turn(ops, dt):
    """9 x 9 planes: lanes 0 .. 16 of avgpool_fwd_kernel add a second element (the nets' last planes have 49 or fewer)"""
    P.avgpool(ops, dt, 2, 64, 9, _recorder("turns", 2))


@pytest.mark.parametrize("Ln", E.DOMINANT_L)
def test_softmax_dominant_logit_past_column_63(ops, Ln):
    """rows whose maximum sits past column 63, more than 89 above every other logit: a maximum taken over the lanes' first turn alone
    overflows expf (ewref.dominant_rows)"""
    x = E.dominant_rows(Ln)
    got = ops.softmax(x)
    ref, A = E.softmax_ref(x)
    w, bad = R.dist_f32(got, ref, A)
    assert bad == 0, "soft-max: %d out of bounds (worst %.3g)" % (bad, w)
    _recorder("turns", len(x))(("softmax dominant", "L=%d" % Ln), w)


@pytest.mark.parametrize("run", EW, ids=EW_IDS)
def test_pools_softmax_fc_ragged(ops, run):
    net, N, (what, arg) = run
    d, rec = DIMS[net], _recorder(net, N)
    Hs = d["input"] // d["init_conv_stride"]
    if what == "maxpool":
        P.maxpool(ops, arg, N, d["init_conv_filters"], Hs, rec)
    elif what == "avgpool":
        P.avgpool(ops, arg, N, d["final_depth"], _last_plane(d), rec)
    elif what == "fc":
        P.fc_gemm(ops, arg, N, d["final_depth"], d["output"], rec)
    elif what == "softmax":
        P.softmax_ce(ops, N, d["output"], rec)
    else:
        P.nhwc_to_nchw(ops, N, d["input"])
