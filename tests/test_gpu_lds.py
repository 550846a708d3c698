"""No kernel reads LDS it did not write: every operator and the trainer with one word written into all LDS of every CU after EVERY launch.

LDS is not cleared between dispatches.  A kernel that reads an LDS word it never wrote (a padded row, a tail k-step, a lane whose LDS-DMA
source was out of range so that nothing landed, a tile image larger than what was staged) reads what the previous kernel on that CU left
there: usually zeros or the same operand, so the error is small, data-dependent and silent.  mi_debug_lds_fill(word) writes `word` into the
whole LDS of every CU (workgroups that own all of a CU's LDS, 8 per CU); mi_debug_lds_fill_mode(1, word) does so after every kernel launch
of the library, between two device synchronises, so each launch of an operator or a training step -- not only the first -- finds `word`
in all LDS it does not write itself.  The fill's workgroups own LDS of their own, so the mode only serialises launches and changes no value.

Three words, in this order:
  0x00000000  the control
  0x47C447C4  finite and positive as fp32 (about 1.0e5) and as each bf16 half (100 352): it passes a ReLU, a max and a compare (where NaN
              is dropped: fmaxf(NaN, 0) = 0 is what a stale 0 gives) and wrecks any sum or index it enters
  0xFFFFFFFF  NaN as fp32 and as both bf16 halves, 255 as a byte, -1 as an int

First the mechanism itself (test_fill_reaches_every_cu, test_probe_sees_another_word, test_mode_fills_after_a_launch): after fill(w) the
read-only probe finds no other word in workgroups x (LDS bytes / 4) words on as many distinct CUs as the device has -- which is also the
measurement that LDS contents survive from one dispatch to the next, the premise of everything below.

Then each case runs on the same inputs under the three words and must satisfy
  (a) every floating-point output is finite under the second and the third word;
  (b) every output is bit-identical across the three words;
  (c) the premise: two control runs are bit-identical (the kernels have no floating-point atomics), asserted once per case family;
and the fill counter must have moved.  Correctness of the values is the business of the per-element files; the operators are run through
their bodies' `_inputs` / `_call` halves (tests/perelement.py) on cheap deterministic operands, generated once per case.

Cases: the lists test_gpu_redzone.py uses (the smallest shapes at which every plan kind ends in a partial tile, where padded rows and
clamped lanes exist): the ragged lists of test_gpu_ragged.py, the planners' corner shapes of test_gpu_ops.py, Adam / SGD / LARS on arenas of
odd length, decode_u8 / resample_u8; the fp32 convolution routes once more per RESNET_MI_IGEMM value in a child process (the direct VALU
kernels and gemm_mfma_kernel); every entry of tests/routes.py with operator cases in a child (tests/route_worker.py, unchanged) under
RESNET_MI_LDS_FILL=47c447c4 and =ffffffff, where the worker's own float64 per-element checkers are the oracle; then the trainer: three
full steps per net, dtype, store policy and optimizer under the three words and with the mode off, bit-identical and finite across the
four; and the uint8-shard loader with the random-resized crop and the prefetch thread, which launches on the copy stream.

Out of reach: LDS words a kernel reads and then discards; a dependence on registers or on global workspace (test_gpu_redzone.py covers
global workspace); races inside a workgroup -- a missing barrier reads the kernel's OWN earlier data, not the fill.
"""
import ctypes as C
import os
import re
import sys
import time

import numpy as np
import pytest

import perelement as P
import routes
import synth
import test_gpu_ragged as G
import test_gpu_redzone as Z
import test_gpu_routes as TR
from test_gpu_bf16 import HYPER
from test_gpu_input_rrc import sweep_boxes
from test_gpu_input_u8 import sweep_plan, write_u8_shards

pytestmark = pytest.mark.gpu

WORDS = [0x00000000, 0x47C447C4, 0xFFFFFFFF]
TOTAL = dict(runs=0, fills=0)
CONTROLLED = set()      # case families whose run-to-run bit identity (two control runs) has been asserted
_flat, _same = Z._flat, Z._same


class Mode:
    """the mode's switch, with the fills counted across switches (the library's counter restarts at every switch-on)"""

    def __init__(self, L):
        self.L, self.word = L, None

    def set(self, word):
        """word None: off"""
        if self.word is not None:
            TOTAL["fills"] += self.L.mi_debug_lds_fills()
        self.word = None
        assert self.L.mi_debug_lds_fill_mode(0 if word is None else 1, word or 0) == 0, self.L.mi_last_error()
        self.word = word

    def fills(self):
        return self.L.mi_debug_lds_fills()


@pytest.fixture(scope="module")
def mode(ops):
    m = Mode(ops.L)
    t0 = time.time()
    try:
        yield m
    finally:
        m.set(None)
        print("\nLDS module: %d runs under the mode, %d fills, %.0f s" % (TOTAL["runs"], TOTAL["fills"], time.time() - t0))


@pytest.fixture
def fm(mode):
    """per test: the mode is off again at the end"""
    mode.L.mi_clear_error()
    try:
        yield mode
        assert mode.L.mi_last_error() == b"", mode.L.mi_last_error()
    finally:
        mode.set(None)
        mode.L.mi_clear_error()


def _finite(what, word, outs):
    for i, b in enumerate(outs):
        if b.dtype.kind == "f":
            assert np.all(np.isfinite(b)), "%s: output %d has %d non-finite elements under word 0x%08x (first at %s)" \
                % (what, i, np.count_nonzero(~np.isfinite(b)), word, np.argwhere(~np.isfinite(b))[0])


def three_words(fm, family, what, call):
    """call() with the mode on under each of WORDS (the control twice, once per family): conditions (a) - (c) of the module docstring"""
    words = WORDS if family in CONTROLLED else WORDS[:1] + WORDS
    outs = []
    for w in words:
        fm.set(w)
        outs.append(_flat(call()))
        TOTAL["runs"] += 1
        assert fm.fills() >= 1, "%s: no fill followed a launch under word 0x%08x" % (what, w)
    fm.set(None)
    if len(words) == 4:
        assert all(_same(a, b) for a, b in zip(outs[0], outs[1])), "%s: two runs under word 0 differ: the premise of the comparison fails" % what
        CONTROLLED.add(family)
    zero = outs[0]
    assert len(zero) > 0
    for w, got in zip(WORDS[1:], outs[-2:]):
        assert len(got) == len(zero)
        _finite(what, w, got)
        for i, (a, b) in enumerate(zip(zero, got)):
            assert _same(a, b), "%s: output %d differs between word 0 and word 0x%08x at %d elements (first at %s)" \
                % (what, i, w, np.count_nonzero(a != b), np.argwhere(a != b)[:1])


# ---------------------------------------------------------------------------------------------------------------------------
# the mechanism itself
def _geometry(L):
    g = (C.c_size_t * 3)()
    assert L.mi_debug_lds_geometry(g) == 0, L.mi_last_error()
    return int(g[0]), int(g[1]), int(g[2])


def _probe(L, word):
    out = (C.c_size_t * 4)()
    assert L.mi_debug_lds_probe(word, out) == 0, L.mi_last_error()
    return dict(workgroups=int(out[0]), cus=int(out[1]), words=int(out[2]), unequal=int(out[3]))


@pytest.mark.parametrize("word", WORDS, ids=["%08x" % w for w in WORDS])
def test_fill_reaches_every_cu(ops, mode, word):
    """after fill(w) a later dispatch finds w in every LDS word of every CU: LDS survives from one dispatch to the next, and the fill covers it"""
    L = ops.L
    lds_bytes, cus, grid = _geometry(L)
    assert lds_bytes == 160 * 1024, "a workgroup may own %d bytes of LDS: not all of a CU's 160 KiB" % lds_bytes
    assert cus >= 1 and grid >= 8 * cus
    mode.set(None)
    assert L.mi_debug_lds_fill(word) == 0, L.mi_last_error()
    got = _probe(L, word)
    print("fill 0x%08x -> probe: %s; LDS bytes per workgroup %d, CUs of the device %d" % (word, got, lds_bytes, cus))
    assert got["workgroups"] == grid
    assert got["cus"] == cus, "the probe's workgroups ran on %d distinct CUs, the device has %d" % (got["cus"], cus)
    assert got["words"] == got["workgroups"] * (lds_bytes // 4)
    assert got["unequal"] == 0, "%d of %d LDS words did not keep the fill until the next dispatch" % (got["unequal"], got["words"])
    again = _probe(L, word)                 # the probe writes no LDS
    assert again["unequal"] == 0 and again["words"] == got["words"]


def test_probe_sees_another_word(ops, mode):
    L = ops.L
    mode.set(None)
    for w, other in ((WORDS[1], WORDS[2]), (WORDS[2], WORDS[0]), (WORDS[0], WORDS[1])):
        assert L.mi_debug_lds_fill(w) == 0
        got = _probe(L, other)
        assert got["unequal"] == got["words"] > 0, (hex(w), hex(other), got)
    assert L.mi_debug_poison_lds() == 0     # the old entry point is the fill with 0xFFFFFFFF
    assert _probe(L, 0xFFFFFFFF)["unequal"] == 0


def test_mode_fills_after_a_launch(ops, fm):
    """with the mode on, one small operator raises the fill counter, and LDS holds the word right after it; off, it does neither"""
    from resnet_amd import binding as B
    L = ops.L
    x = P.pattern((1237,), 3, 1.37)
    for w in WORDS[1:]:
        fm.set(w)
        assert fm.fills() == 0 and _probe(L, w)["unequal"] == 0      # switching on fills once
        assert L.mi_debug_lds_fill(WORDS[0]) == 0                    # something else in LDS: only a fill after the launch can restore w
        y = ops.get_t(ops.dev_t(x, B.MI_DTYPE_BF16), B.MI_DTYPE_BF16)
        n = fm.fills()
        assert n >= 1, "mi_op_convert under the mode: no fill"
        assert _probe(L, w)["unequal"] == 0
        assert np.all(np.isfinite(y))
    fm.set(None)
    n = fm.fills()
    ops.get_t(ops.dev_t(x, B.MI_DTYPE_BF16), B.MI_DTYPE_BF16)
    assert fm.fills() == n


# ---------------------------------------------------------------------------------------------------------------------------
# every operator at the ragged batches
@pytest.mark.parametrize("run", G.CONV, ids=G.CONV_IDS)
def test_conv_route(ops, fm, run):
    net, N, case = run
    inp = P.conv_route_inputs(case, N, P.pattern)
    three_words(fm, "conv %s %s %s" % case[:3], str(run), lambda: P.conv_route_call(ops, case, inp))


@pytest.mark.parametrize("case", Z.SWEEP_CASES, ids=["%s%s_C%d_H%d_K%d_k%d_s%d_N%d" % ((c[2], "_add" if c[8] else "") + c[3:8] + c[9:]) for c in Z.SWEEP_CASES])
def test_conv_shape_sweep(ops, fm, case):
    """the planners' corner shapes of test_gpu_ops.py (SWEEP): fwd, dgrad, dgrad with to_add, wgrad"""
    inp = P.conv_route_inputs(case[:9], case[9], P.pattern)
    three_words(fm, "sweep %s" % case[2], str(case), lambda: P.conv_route_call(ops, case[:9], inp))


@pytest.mark.parametrize("run", G.CONV_BN, ids=G.CONV_BN_IDS)
def test_conv_bn_fwd(ops, fm, run):
    net, N, (case, route) = run
    inp = P.conv_bn_fwd_inputs(case, N, P.pattern)
    three_words(fm, "conv+bn %s %s" % (case[0], route), str(run), lambda: P.conv_bn_fwd_call(ops, case, inp, route))


@pytest.mark.parametrize("run", G.DGRAD_BN, ids=G.DGRAD_BN_IDS)
def test_dgrad_bn_bwd(ops, fm, run):
    net, N, case = run
    inp = P.dgrad_bn_bwd_inputs(case, N, P.pattern)
    three_words(fm, "dgrad+bn' %s" % case[0], str(run), lambda: P.dgrad_bn_bwd_call(ops, case, inp))


@pytest.mark.parametrize("run", G.STEM, ids=G.STEM_IDS)
def test_stem(ops, fm, run):
    net, N, (dt, op, dy_dt) = run
    inp = P.stem_inputs(dt, op, N, G.DIMS[net]["input"], P.pattern)
    three_words(fm, "stem %s %s %d" % (dt, op, dy_dt), str(run), lambda: P.stem_call(ops, dt, op, inp, dy_dt))


@pytest.mark.parametrize("run", G.STEM_BN, ids=G.STEM_BN_IDS)
def test_stem_bn_fwd(ops, fm, run):
    net, N, variant = run
    inp = P.stem_bn_fwd_inputs(variant, N, G.DIMS[net]["input"], P.pattern)
    three_words(fm, "stem+bn %s" % variant, str(run), lambda: P.stem_bn_fwd_call(ops, variant, inp))


@pytest.mark.parametrize("run", G.BN_FWD, ids=G.BN_FWD_IDS)
def test_bn_fwd(ops, fm, run):
    net, N, case = run
    inp = P.bn_fwd_inputs(case, N, cheap=True)

    def call():
        outs = [P.bn_fwd_call(ops, case, inp, form) for form in case[3]]
        if "relu" in case[3]:
            outs.append(P.bn_apply_call(ops, case, inp, outs[0][0], outs[0][1]))
        return outs
    three_words(fm, "bn fwd %s" % case[0], str(run), call)


@pytest.mark.parametrize("run", G.BN_BWD, ids=G.BN_BWD_IDS)
def test_bn_bwd(ops, fm, run):
    net, N, case = run
    inp = P.bn_bwd_inputs(case, N, cheap=True)
    three_words(fm, "bn bwd %s mode %d" % (case[0], case[3]), str(run), lambda: P.bn_bwd_call(ops, case, inp))


@pytest.mark.parametrize("run", G.EW, ids=G.EW_IDS)
def test_pools_softmax_fc(ops, fm, run):
    net, N, (what, arg) = run
    d = G.DIMS[net]
    Hs = d["input"] // d["init_conv_stride"]
    if what == "maxpool":
        inp = P.maxpool_inputs(arg, N, d["init_conv_filters"], Hs, cheap=True)

        def call():
            y, idx = P.maxpool_fwd_call(ops, arg, inp)
            return y, idx, P.maxpool_bwd_call(ops, arg, inp, idx)
    elif what == "avgpool":
        inp = P.avgpool_inputs(arg, N, d["final_depth"], G._last_plane(d), cheap=True)
        call = lambda: P.avgpool_call(ops, arg, inp)
    elif what == "fc":
        inp = P.fc_gemm_inputs(arg, N, d["final_depth"], d["output"], P.pattern)
        call = lambda: P.fc_gemm_call(ops, arg, inp)
    elif what == "softmax":
        inp = P.softmax_ce_inputs(N, d["output"])
        call = lambda: P.softmax_ce_call(ops, inp)
    else:
        inp = P.nhwc_to_nchw_inputs(N, d["input"])
        call = lambda: ops.nhwc_to_nchw(inp)
    three_words(fm, "%s %s" % (what, arg), str(run), call)


# ---------------------------------------------------------------------------------------------------------------------------
# outside the lists
@pytest.mark.parametrize("arena", list(Z.ARENAS))
def test_adam(ops, fm, arena):
    n = Z.ARENAS[arena][-1]
    p, g, m = P.pattern((n,), 1), P.pattern((n,), 2, 0.01), P.pattern((n,), 3, 0.001)
    v = np.abs(P.pattern((n,), 4, 1e-4))
    three_words(fm, "adam", "adam n = %d" % n, lambda: ops.adam(p, g, m, v, 1e-4, 1e-3, 0.9, 0.999, 0.9 ** 3, 0.999 ** 3, 1e-7))


@pytest.mark.parametrize("kind", ["sgd", "lars"])
@pytest.mark.parametrize("arena", list(Z.ARENAS))
def test_momentum_update(ops, fm, arena, kind):
    """the norms of LARS are reduced through LDS"""
    from resnet_amd import binding as B
    offs = Z.ARENAS[arena]
    n = offs[-1]
    w, g, b = P.pattern((n,), 1), P.pattern((n,), 2, 0.01), P.pattern((n,), 3, 0.001)
    is_w = [i % 2 == 0 for i in range(len(offs) - 1)]
    K = {"sgd": B.MI_OPT_SGD, "lars": B.MI_OPT_LARS}[kind]
    three_words(fm, kind, "%s %s" % (kind, arena), lambda: ops.momentum_update(K, w, g, b, offs, is_w, 0.1, 5e-5, 0.9, 0.001))


@pytest.mark.parametrize("dim_in,dim_out,n", [(37, 30, 33), (257, 224, 1)])
def test_decode_and_resample(ops, fm, dim_in, dim_out, n):
    """the input kernels keep byte rows and tables in LDS: 0xFF there is 255, 0x47C447C4 the bytes c4 47 c4 47"""
    rng = np.random.RandomState(dim_in * 1000 + dim_out + n)
    src = rng.randint(0, 256, size=(n, dim_in, dim_in, 3), dtype=np.uint8)
    pl = sweep_plan(n, dim_in - dim_out, rng)
    boxes = sweep_boxes(n, dim_in, dim_out, rng)
    three_words(fm, "decode", "decode %s" % ((dim_in, dim_out, n),), lambda: ops.decode_u8(src, pl, dim_out))
    three_words(fm, "resample", "resample %s" % ((dim_in, dim_out, n),), lambda: ops.resample_u8(src, boxes, dim_out))


@pytest.mark.parametrize("igemm", ["0", "1"])
def test_conv_routes_on_the_other_kernel_routes(igemm):
    """RESNET_MI_IGEMM = 0 / 1: the fp32 convolutions on the direct VALU kernels and gemm_mfma_kernel, which stage through LDS tiles of
    their own.  The routes are read once per process: a child per value runs the fp32 convolution-route cases of this file"""
    here = os.path.dirname(os.path.abspath(__file__))
    r = TR.run_child("conv routes, RESNET_MI_IGEMM=" + igemm,
                     [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "test_conv_route and f32_default",
                      "-p", "no:cacheprovider"], dict(RESNET_MI_IGEMM=igemm), 900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == sum(1 for _, _, c in G.CONV if c[:2] == ("f32", "default")), r.stdout[-500:]


@pytest.mark.parametrize("word", ["47c447c4", "ffffffff"])
@pytest.mark.parametrize("key", [e["key"] for e in TR.OP_ENTRIES])
def test_route_switch_cases_under_the_fill(key, word, tmp_path):
    """every entry of tests/routes.py with operator cases: route_worker.py ops, unchanged, with the mode on from the environment.  Its
    float64 per-element checkers are the oracle (a stale 1e5 or NaN cannot stay inside their bounds); it writes OUT.json only if every
    case passed"""
    import json
    e = routes.by_key(key)
    out = str(tmp_path / "out.json")
    r = TR.run_child("operators %s under LDS word %s" % (key, word), [sys.executable, TR.WORKER, "ops", out, key],
                     dict(routes.env_of(e), RESNET_MI_LDS_FILL=word), 600)
    assert r.returncode == 0, "%s\n%s" % (key, r.stdout[-3000:] + r.stderr[-3000:])
    with open(out) as f:
        got = json.load(f)
    assert got["checked"] == len(e["cases"]) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# the trainer: several hundred launches per step, every one after the first sees its predecessor's LDS
STEPS = 3
# (net, dtype, store policy, optimizer): FAST everywhere, RECOMPUTE_BN once per dtype, SGD and LARS once
TRAINERS = [(net, dt, "FAST", "adam") for net in Z.NETS for dt in ("f32", "bf16")] + \
           [("R50", "f32", "RECOMPUTE_BN", "adam"), ("R50", "bf16", "RECOMPUTE_BN", "adam"), ("C1S", "f32", "FAST", "sgd"), ("C1S", "bf16", "FAST", "lars")]


def _train(fm, word, net, dt, policy, opt):
    """three full steps on the synthetic source with the mode set BEFORE the trainer exists -> (losses, predictions, state)"""
    from resnet_amd import Trainer
    from resnet_amd import binding as B
    dims, batch = Z.NETS[net]
    fm.set(word)
    tr = Trainer(dims, batch, **HYPER)
    try:
        tr.set_store_policy(getattr(B, "MI_STORE_" + policy))
        tr.set_dtype(B.MI_DTYPE_BF16 if dt == "bf16" else B.MI_DTYPE_F32)
        if opt != "adam":
            tr.set_optimizer(opt)
        tr.source_synthetic()
        out = []
        for step in range(STEPS):
            before = fm.fills()
            loss, _ = tr.step()
            tr.check()
            assert tr.check_errors() == 0
            out += [np.float64(loss), tr.pred()]
            assert word is None or fm.fills() > before, "step %d: no fill" % step
        out += [tr.get(w, i) for w in ("params", "means", "vars") for i in range(tr.n_locations)]
    finally:
        tr.close()
    if word is not None:
        TOTAL["runs"] += 1
    fm.set(None)
    return out


def _name(i):
    return ("loss", "predictions")[i % 2] + " of step %d" % (i // 2) if i < 2 * STEPS else "state tensor %d" % (i - 2 * STEPS)


@pytest.mark.parametrize("cfg", TRAINERS, ids=["-".join(c) for c in TRAINERS])
def test_trainer_three_steps(ops, fm, cfg):
    runs = [_train(fm, w, *cfg) for w in WORDS + [None]]
    zero = runs[0]
    for w, got in zip(WORDS[1:] + [None], runs[1:]):
        tag = "the mode off" if w is None else "word 0x%08x" % w
        assert len(got) == len(zero)
        for i, (a, b) in enumerate(zip(zero, got)):
            assert np.all(np.isfinite(b)), "%s: %s is not finite under %s" % (cfg, _name(i), tag)
            assert _same(np.asarray(a), np.asarray(b)), "%s: %s differs between word 0 and %s" % (cfg, _name(i), tag)


def test_loader_rrc_prefetched(ops, fm, tmp_path):
    """the uint8-shard loader with the random-resized crop and the prefetch thread: the decode / resample kernels launch on the copy stream,
    from another thread, under the mode; one pass over two tiny shards with full training steps between the loads"""
    from resnet_amd import Trainer
    din, per_shard, batch = 40, 8, 4
    _, u8, _ = write_u8_shards(str(tmp_path), 2, per_shard, din, synth.C1_DIMS["input"])

    def run(word):
        fm.set(word)
        tr = Trainer(synth.C1_DIMS, batch, seed=1236, shard_n_images=per_shard)
        out = []
        try:
            tr.L.mi_trainer_set_input_reset(tr.t, 1)
            tr.source_shards_u8(u8, din, augment="rrc", flip=True, seed=4242, prefetch=True, scale=(0.2, 1.0), ratio=(0.5, 2.0))
            for step in range(2 * per_shard // batch):
                tr.load_new_batch()
                assert tr.L.mi_batch_last_status(tr.c_batch) == 0
                out += [tr.last_boxes(), tr.activation("input")]
                tr.forward()
                out.append(np.float64(tr.loss()[0]))
                tr.backward()
                tr.update()
                tr.check()
        finally:
            tr.close()
        if word is not None:
            assert fm.fills() >= 1
            TOTAL["runs"] += 1
        fm.set(None)
        return out

    runs = [run(w) for w in WORDS + [None]]
    for w, got in zip(WORDS[1:] + [None], runs[1:]):
        for i, (a, b) in enumerate(zip(runs[0], got)):
            assert np.all(np.isfinite(b)), "loader output %d is not finite under %s" % (i, w)
            assert _same(np.asarray(a), np.asarray(b)), "loader output %d differs between word 0 and %s" % (i, "the mode off" if w is None else hex(w))
