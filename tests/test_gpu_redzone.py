"""Kernels stay inside their tensors: every operator and the trainer under the red-zone mode of the device allocator (mi_debug_redzone).

While the mode is on, every device allocation of the library (operator tensors, the workspaces ops.c makes per call, every trainer tensor,
the loader's and the optimizer's buffers) is zone | payload | zone with the whole of it filled with one byte value; the zones are compared
with that value when the allocation is freed and in mi_debug_redzone_check.  Nothing here provokes a fault: every access, the planted damage
of the self-test included, lies inside an allocation of this process, and the zones make a stray access LESS likely to leave one.

Each case runs on the same inputs under fill 0x00 (the control: what a fresh hipMalloc usually holds) and under fill 0xFF (NaN as fp32 and
as bf16, -1 as an int), and must satisfy
  1. no zone byte changed (out-of-bounds writes of the kernel or of anything ops.c launches for it; the per-call workspaces, statistics
     partials, re-laid weights and channel-last operands are verified when ops.c frees them), and no byte of the MI_GUARD slack mi_malloc
     leaves around every operator tensor changed either (`_GuardedArray`: kernels may read that slack, none may write it);
  2. every output of the 0xFF run is finite (an output element never written or accumulated into; a masked lane that multiplies the
     guard bytes by zero instead of selecting);
  3. every output is bit-identical between the two fills (any dependence on bytes outside the tensors passed in: guard bytes, zones,
     uninitialised workspace).  The kernels have no floating-point atomics, so two runs of a correct kernel agree bit for bit; that premise
     is asserted once per case family with a second 0x00 run.
Correctness of the values is the business of the per-element files; the operators are run through their bodies' `_inputs` / `_call` halves
(tests/perelement.py) on cheap deterministic operands, generated once per case.

Cases: the lists and batches of test_gpu_ragged.py (the smallest at which every plan kind ends in a partial tile), plus Adam / SGD / LARS on
arenas of odd length, decode_u8 / resample_u8 at the shapes whose rows end in guarded 16-byte loads, mi_op_convert, the planners' corner
shapes of test_conv_shape_sweep, and the fp32 convolution routes once more per RESNET_MI_IGEMM value in a child process (the direct VALU
kernels and gemm_mfma_kernel).  Then the trainer, which allocates once and reuses: three full steps of C1S, C4I and ResNet-50 per dtype,
store policy and optimizer, with the mode on before the trainer exists, under both fills and with the mode off -- losses, predictions,
parameters and optimizer state bit-identical and finite across the three; and the uint8-shard loader with the random-resized crop and the
prefetch thread.

ZONE = 256 KiB on each side.  It is a choice, not a measurement: it only has to exceed any plausible contiguous overrun (a full 128-column
fp32 tile row is 512 bytes, a 7 x 7 fp32 plane 196 bytes, the largest tile of any kernel here 128 x 128 x 4 = 64 KiB) and stay small
enough that ResNet-50 at batch 8 with its several hundred allocations fits many times over.  Out of reach of this method: a strided
overrun that jumps clear over the zone, and reads that are loaded and then discarded (they change nothing and, inside the zone, fault
nothing).
"""
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import convref as R
import ewref as E
import perelement as P
import synth
import test_gpu_ragged as G
from test_gpu_bf16 import HYPER
from test_gpu_input_rrc import sweep_boxes
from test_gpu_input_u8 import sweep_plan, write_u8_shards
from test_gpu_ops import SWEEP

pytestmark = pytest.mark.gpu

ZONE = 256 * 1024
TOTAL = dict(allocs=0, zone_bytes=0, runs=0)
CONTROLLED = set()      # case families whose run-to-run bit identity (two 0x00 runs) has been asserted
GUARD_DAMAGE = []       # findings of _GuardedArray.free
DESC = re.compile(r"allocation #(\d+) of (\d+) bytes, (front|back) zone, offsets (-?\d+)\.\.(-?\d+) from the payload's (start|end), (\d+) bytes")


class Zone:
    """the mode's switch with the counters kept across switches (mi_debug_redzone restarts the library's own at every switch-on)"""

    def __init__(self, L):
        self.L, self.fill, self.seen = L, None, (0, 0)

    def _harvest(self):
        a, b, live = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self.L.mi_debug_redzone_stats(C.byref(a), C.byref(b), C.byref(live))
        TOTAL["allocs"] += a.value - self.seen[0]
        TOTAL["zone_bytes"] += b.value - self.seen[1]
        self.seen = (a.value, b.value)
        return live.value

    def set(self, fill):
        """fill None: off"""
        self._harvest()
        assert self.L.mi_debug_redzone(0 if fill is None else ZONE, fill or 0) == 0
        if fill is not None:
            self.seen = (0, 0)
        self.fill = fill

    def damaged(self):
        n = self.L.mi_debug_redzone_check()
        self._harvest()
        return n

    def check(self, what):
        n = self.damaged()
        assert n == 0, "%s: %d damaged allocation(s); first: %s" % (what, n, self.L.mi_last_error().decode())
        assert not GUARD_DAMAGE, "%s: MI_GUARD slack written: %s" % (what, GUARD_DAMAGE[0])
        assert self.L.mi_last_error() == b"", "%s: %s" % (what, self.L.mi_last_error().decode())


@pytest.fixture(scope="module")
def zone(ops):
    """switches the mode off at the end of the module; under it every DeviceArray also checks its MI_GUARD slack when it is freed"""
    from resnet_amd import binding as B
    from resnet_amd import ops as O
    z = Zone(ops.L)
    t0 = time.time()
    init, free = O.DeviceArray.__init__, O.DeviceArray.free

    def guarded_init(self, lib, arr=None, shape=None, dtype=np.float32):
        self._fill = z.fill
        init(self, lib, arr, shape, dtype)

    def guarded_free(self):
        fill = getattr(self, "_fill", None)
        if self.ptr and fill is not None:
            buf = np.empty(B.MI_GUARD, np.uint8)
            for side, at in (("front", self.ptr - B.MI_GUARD), ("back", self.ptr + max(self.nbytes, 4))):
                self.L.mi_copy_to_host(buf.ctypes.data, at, B.MI_GUARD)
                bad = np.flatnonzero(buf != fill)
                if bad.size:
                    GUARD_DAMAGE.append("%s guard of a %s %s tensor: %d bytes, offsets %d..%d" % (side, self.shape, self.dtype, bad.size, bad[0], bad[-1]))
        free(self)

    O.DeviceArray.__init__, O.DeviceArray.free = guarded_init, guarded_free
    try:
        yield z
    finally:
        O.DeviceArray.__init__, O.DeviceArray.free = init, free
        z.set(None)
        ops.L.mi_clear_error()
        print("\nred-zone module: %d runs, %d allocations checked, %.1f MB of zone bytes compared, %.0f s"
              % (TOTAL["runs"], TOTAL["allocs"], TOTAL["zone_bytes"] / 1e6, time.time() - t0))


@pytest.fixture
def rz(zone):
    """per test: the zones are intact at the end, and the test did not check nothing"""
    del GUARD_DAMAGE[:]
    zone.L.mi_clear_error()
    before = TOTAL["allocs"]
    yield zone
    try:
        zone.check("end of test")
        assert TOTAL["allocs"] > before, "no padded allocation was checked"
    finally:
        zone.set(None)
        zone.L.mi_clear_error()


def _flat(out):
    """the outputs of one run as a list of arrays"""
    if isinstance(out, np.ndarray):
        return [out]
    if isinstance(out, (tuple, list)):
        return [a for o in out for a in _flat(o)]
    return [np.asarray(out)]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def both_fills(rz, family, what, call):
    """call() under 0x00 and under 0xFF (and under 0x00 again, once per family): conditions 1 - 3 of the module docstring"""
    fills = [0x00, 0xFF] if family in CONTROLLED else [0x00, 0x00, 0xFF]
    outs = []
    for fill in fills:
        rz.set(fill)
        outs.append(_flat(call()))
        TOTAL["runs"] += 1
        rz.check("%s, fill 0x%02x" % (what, fill))
    if len(fills) == 3:
        assert all(_same(a, b) for a, b in zip(outs[0], outs[1])), "%s: two runs under fill 0x00 differ: the premise of the comparison fails" % what
        CONTROLLED.add(family)
    zero, nan = outs[0], outs[-1]
    assert len(zero) == len(nan) and len(zero) > 0
    for i, (a, b) in enumerate(zip(zero, nan)):
        if b.dtype.kind == "f":
            assert np.all(np.isfinite(b)), "%s: output %d has %d non-finite elements under fill 0xFF (first at %s)" \
                % (what, i, np.count_nonzero(~np.isfinite(b)), np.argwhere(~np.isfinite(b))[0])
        assert _same(a, b), "%s: output %d differs between fill 0x00 and fill 0xFF at %d elements (first at %s)" \
            % (what, i, np.count_nonzero(a != b), np.argwhere(a != b)[:1])


# ---------------------------------------------------------------------------------------------------------------------------
# the mechanism itself
def _poke(L, at, value):
    b = np.array([value], np.uint8)
    L.mi_copy_to_device(at, b.ctypes.data, 1)


def _report(L):
    m = DESC.search(L.mi_last_error().decode())
    assert m, L.mi_last_error()
    serial, nbytes, side, first, last, ref, n = m.groups()
    return int(nbytes), side, int(first), int(last), ref, int(n)


def test_refuses_a_zone_that_would_move_the_alignment(ops, zone):
    L = ops.L
    L.mi_clear_error()
    assert L.mi_debug_redzone(1000, 0) == -1 and b"4096" in L.mi_last_error()
    L.mi_clear_error()


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_planted_damage_is_reported(ops, zone, fill):
    """one byte written just behind / just in front of a small tensor's allocation (inside the zone, so inside the process's own memory) is
    reported with its side, offset and size: live, freed before the check, and forgotten when the mode is switched on again.  A DeviceArray's
    pointer lies MI_GUARD inside the allocation (mi_malloc), so the payload the report speaks of is [ptr - MI_GUARD, ptr + nbytes + MI_GUARD)"""
    from resnet_amd import binding as B
    L = ops.L
    L.mi_clear_error()
    del GUARD_DAMAGE[:]
    GU = B.MI_GUARD
    try:
        zone.set(fill)
        a = ops.dev(np.arange(16, dtype=np.float32))
        payload = a.nbytes + 2 * GU
        assert zone.damaged() == 0 and L.mi_last_error() == b""
        _poke(L, a.ptr + a.nbytes + GU, fill ^ 0x5A)                 # the first byte of the back zone
        assert zone.damaged() == 1
        assert _report(L) == (payload, "back", 0, 0, "end", 1)
        assert zone.damaged() == 1                                   # sticky, and one allocation is counted once
        assert np.array_equal(a.get(), np.arange(16, dtype=np.float32))
        a.free()
        assert zone.damaged() == 1                                   # freed ones stay counted
        L.mi_clear_error()
        assert zone.damaged() == 1 and _report(L)[1] == "back"       # ... and described, after the channel was cleared
        L.mi_clear_error()

        zone.set(fill)                                               # switched on again: the count starts at zero
        assert zone.damaged() == 0 and L.mi_last_error() == b""
        b = ops.dev(np.arange(16, dtype=np.float32))
        _poke(L, b.ptr - GU - 1, fill ^ 0x5A)                        # the last byte of the front zone
        assert zone.damaged() == 1
        assert _report(L) == (payload, "front", -1, -1, "start", 1)
        b.free()
        L.mi_clear_error()

        zone.set(fill)
        c = ops.dev(np.arange(16, dtype=np.float32))
        _poke(L, c.ptr + c.nbytes + GU + 4095, fill ^ 0xFF)
        _poke(L, c.ptr + c.nbytes + GU + 7, fill ^ 0x01)
        c.free()                                                     # freed before any check: found at the free
        assert zone.damaged() == 1
        assert _report(L) == (payload, "back", 7, 4095, "end", 2)
        L.mi_clear_error()

        d = ops.dev(np.arange(16, dtype=np.float32))                 # padded under this fill, freed after the mode went off
        zone.set(None)
        e = ops.dev(np.arange(16, dtype=np.float32))                 # not padded
        _poke(L, d.ptr + d.nbytes + GU + 1, fill ^ 0x10)
        d.free()
        e.free()
        assert zone.damaged() == 2 and L.mi_last_error() != b""
        L.mi_clear_error()
        zone.set(fill)
        assert zone.damaged() == 0 and L.mi_last_error() == b""
        assert not GUARD_DAMAGE
    finally:
        zone.set(None)
        L.mi_clear_error()


def test_guard_damage_is_seen(ops, zone):
    """the MI_GUARD slack of an operator tensor (readable by the bf16 kernels, written by none) is checked when the tensor is freed"""
    del GUARD_DAMAGE[:]
    try:
        zone.set(0xFF)
        a = ops.dev(np.zeros(5, np.float32))
        _poke(ops.L, a.ptr + a.nbytes + 3, 0)
        a.free()
        assert len(GUARD_DAMAGE) == 1 and "back guard" in GUARD_DAMAGE[0] and "offsets 3..3" in GUARD_DAMAGE[0]
        assert zone.damaged() == 0
    finally:
        del GUARD_DAMAGE[:]
        zone.set(None)


# ---------------------------------------------------------------------------------------------------------------------------
# every operator at the ragged batches
@pytest.mark.parametrize("run", G.CONV, ids=G.CONV_IDS)
def test_conv_route(ops, rz, run):
    net, N, case = run
    inp = P.conv_route_inputs(case, N, P.pattern)
    both_fills(rz, "conv %s %s %s" % case[:3], str(run), lambda: P.conv_route_call(ops, case, inp))


SWEEP_CASES = [("f32", "default", op, C_, H, K, k, s, where, N) for (C_, H, K, k, s, N) in SWEEP
               for op, where in (("fwd", ""), ("dgrad", ""), ("dgrad", "red"), ("wgrad", ""))]


@pytest.mark.parametrize("case", SWEEP_CASES, ids=["%s%s_C%d_H%d_K%d_k%d_s%d_N%d" % ((c[2], "_add" if c[8] else "") + c[3:8] + c[9:]) for c in SWEEP_CASES])
def test_conv_shape_sweep(ops, rz, case):
    """the planners' corner shapes of test_gpu_ops.py: 2 x 2 and 3 x 3 images, 64-column half tiles, N = 40, channel counts that fall back to
    the direct kernels for one operator only"""
    inp = P.conv_route_inputs(case[:9], case[9], P.pattern)
    both_fills(rz, "sweep %s" % case[2], str(case), lambda: P.conv_route_call(ops, case[:9], inp))


@pytest.mark.parametrize("run", G.CONV_BN, ids=G.CONV_BN_IDS)
def test_conv_bn_fwd(ops, rz, run):
    net, N, (case, route) = run
    inp = P.conv_bn_fwd_inputs(case, N, P.pattern)
    both_fills(rz, "conv+bn %s %s" % (case[0], route), str(run), lambda: P.conv_bn_fwd_call(ops, case, inp, route))


@pytest.mark.parametrize("run", G.DGRAD_BN, ids=G.DGRAD_BN_IDS)
def test_dgrad_bn_bwd(ops, rz, run):
    net, N, case = run
    inp = P.dgrad_bn_bwd_inputs(case, N, P.pattern)
    both_fills(rz, "dgrad+bn' %s" % case[0], str(run), lambda: P.dgrad_bn_bwd_call(ops, case, inp))


@pytest.mark.parametrize("run", G.STEM, ids=G.STEM_IDS)
def test_stem(ops, rz, run):
    net, N, (dt, op, dy_dt) = run
    inp = P.stem_inputs(dt, op, N, G.DIMS[net]["input"], P.pattern)
    both_fills(rz, "stem %s %s %d" % (dt, op, dy_dt), str(run), lambda: P.stem_call(ops, dt, op, inp, dy_dt))


@pytest.mark.parametrize("run", G.STEM_BN, ids=G.STEM_BN_IDS)
def test_stem_bn_fwd(ops, rz, run):
    net, N, variant = run
    inp = P.stem_bn_fwd_inputs(variant, N, G.DIMS[net]["input"], P.pattern)
    both_fills(rz, "stem+bn %s" % variant, str(run), lambda: P.stem_bn_fwd_call(ops, variant, inp))


@pytest.mark.parametrize("run", G.BN_FWD, ids=G.BN_FWD_IDS)
def test_bn_fwd(ops, rz, run):
    net, N, case = run
    inp = P.bn_fwd_inputs(case, N, cheap=True)

    def call():
        outs = [P.bn_fwd_call(ops, case, inp, form) for form in case[3]]
        if "relu" in case[3]:
            outs.append(P.bn_apply_call(ops, case, inp, outs[0][0], outs[0][1]))
        return outs
    both_fills(rz, "bn fwd %s" % case[0], str(run), call)


@pytest.mark.parametrize("run", G.BN_BWD, ids=G.BN_BWD_IDS)
def test_bn_bwd(ops, rz, run):
    net, N, case = run
    inp = P.bn_bwd_inputs(case, N, cheap=True)
    both_fills(rz, "bn bwd %s mode %d" % (case[0], case[3]), str(run), lambda: P.bn_bwd_call(ops, case, inp))


@pytest.mark.parametrize("run", G.EW, ids=G.EW_IDS)
def test_pools_softmax_fc(ops, rz, run):
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
    both_fills(rz, "%s %s" % (what, arg), str(run), call)


# ---------------------------------------------------------------------------------------------------------------------------
# outside the lists
@pytest.mark.parametrize("n", [1, 3, 1237, 65536 + 5])
def test_convert(ops, rz, n):
    """mi_op_convert both ways at lengths that are no multiple of the vector width"""
    from resnet_amd import binding as B
    x = P.pattern((n,), 3, 1.37)
    both_fills(rz, "convert", "convert n = %d" % n, lambda: ops.get_t(ops.dev_t(x, B.MI_DTYPE_BF16), B.MI_DTYPE_BF16))


# tensor lengths of an arena: the operator takes a tensor's length from the gap between two offsets, and offsets are multiples of 4 floats
# (mi_optim_init), so only the last tensor's length is free: 1 float in the first arena, an odd length in the second; the gaps are no
# multiples of the kernels' 1024-float chunk
ARENAS = {"last_is_1": [0, 4, 1032, 1036, 5144, 5145], "last_is_odd": [0, 1028, 1032, 4140, 4140 + 1237]}


@pytest.mark.parametrize("arena", list(ARENAS))
def test_adam(ops, rz, arena):
    n = ARENAS[arena][-1]
    p, g, m = P.pattern((n,), 1), P.pattern((n,), 2, 0.01), P.pattern((n,), 3, 0.001)
    v = np.abs(P.pattern((n,), 4, 1e-4))
    both_fills(rz, "adam", "adam n = %d" % n, lambda: ops.adam(p, g, m, v, 1e-4, 1e-3, 0.9, 0.999, 0.9 ** 3, 0.999 ** 3, 1e-7))


@pytest.mark.parametrize("kind", ["sgd", "lars"])
@pytest.mark.parametrize("arena", list(ARENAS))
def test_momentum_update(ops, rz, arena, kind):
    from resnet_amd import binding as B
    offs = ARENAS[arena]
    n = offs[-1]
    w, g, b = P.pattern((n,), 1), P.pattern((n,), 2, 0.01), P.pattern((n,), 3, 0.001)
    is_w = [i % 2 == 0 for i in range(len(offs) - 1)]
    K = {"sgd": B.MI_OPT_SGD, "lars": B.MI_OPT_LARS}[kind]
    both_fills(rz, kind, "%s %s" % (kind, arena), lambda: ops.momentum_update(K, w, g, b, offs, is_w, 0.1, 5e-5, 0.9, 0.001))


@pytest.mark.parametrize("dim_in,dim_out,n", [(37, 30, 33), (257, 224, 1)])
def test_decode_and_resample(ops, rz, dim_in, dim_out, n):
    """the input kernels at the shapes whose last source rows end in the guarded 16-byte loads (test_decode_sweep, test_resample_sweep)"""
    rng = np.random.RandomState(dim_in * 1000 + dim_out + n)
    src = rng.randint(0, 256, size=(n, dim_in, dim_in, 3), dtype=np.uint8)
    pl = sweep_plan(n, dim_in - dim_out, rng)
    boxes = sweep_boxes(n, dim_in, dim_out, rng)
    both_fills(rz, "decode", "decode %s" % ((dim_in, dim_out, n),), lambda: ops.decode_u8(src, pl, dim_out))
    both_fills(rz, "resample", "resample %s" % ((dim_in, dim_out, n),), lambda: ops.resample_u8(src, boxes, dim_out))


@pytest.mark.parametrize("mode", ["0", "1"])
def test_conv_routes_on_the_other_kernel_routes(mode):
    """RESNET_MI_IGEMM = 0 / 1 (test_gpu_ops.py::test_conv_parity_on_the_other_kernel_routes): the fp32 convolutions on the direct VALU
    kernels and gemm_mfma_kernel, which stage through LDS tiles of their own.  The routes are read once per process: a child per value
    runs the fp32 convolution-route cases of this file"""
    env = dict(os.environ, RESNET_MI_IGEMM=mode)
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "test_conv_route and f32_default",
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=900, cwd=os.path.dirname(here))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == sum(1 for _, _, c in G.CONV if c[:2] == ("f32", "default")), r.stdout[-500:]


# ---------------------------------------------------------------------------------------------------------------------------
# the trainer: allocated once, reused at every step
STEPS = 3
NETS = {"C1S": (synth.C1S_DIMS, 4), "C4I": (synth.C4I_DIMS, 4), "R50": (synth.R50_DIMS, 8)}
# (net, dtype, store policy, optimizer): the FULL policy exists in fp32 only
TRAINERS = [(net, dt, pol, "adam") for net in NETS for dt, pols in (("f32", ("FAST", "RECOMPUTE_BN", "FULL")), ("bf16", ("FAST", "RECOMPUTE_BN")))
            for pol in pols] + [("C1S", "f32", "FAST", "sgd"), ("C1S", "bf16", "FAST", "lars")]


def _train(z, fill, net, dt, policy, opt):
    """three full steps on the synthetic source with the mode set BEFORE the trainer exists -> (losses, predictions, state)"""
    from resnet_amd import Trainer
    from resnet_amd import binding as B
    dims, batch = NETS[net]
    z.set(fill)
    what = "%s %s %s %s, fill %s" % (net, dt, policy, opt, "off" if fill is None else "0x%02x" % fill)
    tr = Trainer(dims, batch, **HYPER)
    try:
        tr.set_store_policy(getattr(B, "MI_STORE_" + policy))
        tr.set_dtype(B.MI_DTYPE_BF16 if dt == "bf16" else B.MI_DTYPE_F32)
        if opt != "adam":
            tr.set_optimizer(opt)
        tr.source_synthetic()
        out = []
        for step in range(STEPS):
            loss, _ = tr.step()
            tr.check()
            assert tr.check_errors() == 0
            out += [np.float64(loss), tr.pred()]
            if fill is not None:
                z.check("%s, step %d" % (what, step))
        out += [tr.get(w, i) for w in ("params", "means", "vars") for i in range(tr.n_locations)]
    finally:
        tr.close()
    if fill is not None:
        z.check("%s, after close" % what)
        TOTAL["runs"] += 1
    return out


def _compare_trainers(z, what, run):
    zero, nan, off = run(0x00), run(0xFF), run(None)
    assert len(zero) == len(nan) == len(off)
    for i, (a, b, c) in enumerate(zip(zero, nan, off)):
        name = ("loss", "predictions")[i % 2] + " of step %d" % (i // 2) if i < 2 * STEPS else "state tensor %d" % (i - 2 * STEPS)
        assert np.all(np.isfinite(b)), "%s: %s is not finite under fill 0xFF" % (what, name)
        assert _same(np.asarray(a), np.asarray(b)), "%s: %s differs between fill 0x00 and fill 0xFF" % (what, name)
        assert _same(np.asarray(a), np.asarray(c)), "%s: %s differs between fill 0x00 and the mode off" % (what, name)


@pytest.mark.parametrize("cfg", TRAINERS, ids=["-".join(c) for c in TRAINERS])
def test_trainer_three_steps(ops, rz, cfg):
    """does the trainer anywhere rely on hipMalloc returning zeros, or a rolling buffer, shared scratch or statistics table run into its
    neighbour: the second and third steps are the ones that see reused buffers"""
    _compare_trainers(rz, str(cfg), lambda fill: _train(rz, fill, *cfg))


def test_loader_rrc_prefetched(ops, rz, tmp_path):
    """the uint8-shard loader with the random-resized crop and the prefetch thread (which allocates too): decode / resample kernels, the
    staging and plan buffers under the mode; one pass over two tiny shards with full training steps between the loads"""
    from resnet_amd import Trainer
    din, per_shard, batch = 40, 8, 4
    _, u8, _ = write_u8_shards(str(tmp_path), 2, per_shard, din, synth.C1_DIMS["input"])

    def run(fill):
        rz.set(fill)
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
                if fill is not None:
                    rz.check("loader step %d, fill 0x%02x" % (step, fill))
        finally:
            tr.close()
        if fill is not None:
            rz.check("loader after close, fill 0x%02x" % fill)
            TOTAL["runs"] += 1
        return out

    zero, nan, off = run(0x00), run(0xFF), run(None)
    for i, (a, b, c) in enumerate(zip(zero, nan, off)):
        assert np.all(np.isfinite(b)), "loader output %d is not finite under fill 0xFF" % i
        assert _same(np.asarray(a), np.asarray(b)) and _same(np.asarray(a), np.asarray(c)), "loader output %d differs between the fills / the mode off" % i
