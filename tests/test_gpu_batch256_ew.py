"""The element-wise half of the training step at the benchmark's batch (256), element by element against float64 references
(tests/ewref.py, bounds of tests/convref.py): batch norm forward (statistics; apply with ReLU, without, with the shortcut add, and the bf16
dual write of a channel-last copy) and backward (modes 1, 3, 0) at every (C, H) of ResNet-50 in every storage pair the trainer uses,
max-pool 3x3 / 2 over the stem output, average pool, soft-max and the cross-entropy derivative, Adam over an arena of ResNet-50's size,
and the NHWC -> NCHW conversion of the batch.

At N = 256 the kernels run the plans the small-batch tests never reach: 32 statistics splits at C = 64 (1 at C = 2048), the widest vectors,
and on 7x7 planes the straddle form, where a vector that runs into the next channel's plane (from C - 1 into channel 0 of the next image)
takes that channel's scalars.  Per-element checks run on convref's slabs (every channel of a few images, every image of the first, last and
6 seeded channels of every 64-channel block); max-pool, the channel-last copies, the pool gradients, ce_deriv and the conversion are
compared bit for bit over whole tensors.  The bodies are tests/perelement.py's.
"""
import os
import resource
import time

import numpy as np
import pytest

import convref as R
import ewref as E
import perelement as P
import synth

pytestmark = pytest.mark.gpu

N = R.N256
F = np.float32
F32, BF16 = P.F32, P.BF16
WORST = {}  # (kernel, form) -> worst distance: 2^-24 A (fp32 outputs, reductions) or bf16 ulps (bf16 outputs); printed at the end


def _record(key, worst):
    WORST[key] = max(WORST.get(key, 0.0), worst)


@pytest.fixture(scope="module", autouse=True)
def _threads():
    R.set_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))
    t0 = time.time()
    yield
    print("\nworst distance per kernel and form at N = %d (x 2^-24 A, or bf16 ulps where the output is bf16); module %.0f s"
          % (N, time.time() - t0))
    for key in sorted(WORST):
        print("  %-34s %-22s %.3g" % (key + (WORST[key],)))


@pytest.fixture(autouse=True)
def _host_peak(request):
    """the process's peak host memory after each test (the module is held to about 10 GB)"""
    yield
    print(" [peak host RSS %.2f GB]" % (resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20))


# ---------------------------------------------------------------------------------------------------------------------------
FWD = E.bn_fwd_cases()


@pytest.mark.parametrize("case", FWD, ids=["%s_C%d_H%d" % c[:3] for c in FWD])
def test_bn_fwd_at_batch_256(ops, case):
    """statistics (bn_stats -> bn_finalize) per channel against float64 over all N * P samples; every apply form of this shape against the
    float64 apply with the kernel's statistics; RECOMPUTE_BN's apply from given statistics; the channel-last copies bit for bit"""
    P.bn_fwd(ops, case, N, _record)


# ---------------------------------------------------------------------------------------------------------------------------
BWD = E.bn_bwd_cases()


@pytest.mark.parametrize("case", BWD, ids=["%s_C%d_H%d_mode%d" % c for c in BWD])
def test_bn_bwd_at_batch_256(ops, case):
    """mi_op_bn_bwd_t: dbeta, dgamma to C_FACTOR 2^-24 sum|terms| against float64 sums of the gated gradient; dx against the float64
    formula from those sums; mode 3's gated dy bit for bit (mask > 0 ? dy : 0).  The statistics are given, as the trainer gives the stored
    ones; means are bf16 numbers so that x == mean can be planted in either storage type"""
    P.bn_bwd(ops, case, N, _record)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_maxpool_3x3s2_at_batch_256(ops, dt):
    """the stem's max-pool (256 x 64 x 112^2, maxpool_fwd_3x3s2_kernel / maxpool_bwd_3x3s2_kernel): values, arg-max indices and dx bit for
    bit against the documented rule, on post-ReLU input with planted ties inside windows and across the overlaps of neighbouring windows"""
    P.maxpool(ops, dt, N, 64, 112, _record)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_avgpool_at_batch_256(ops, dt):
    """256 x 2048 x 7^2: the forward (49-term sums) against float64; the backward dy / 49 in fp32, stored: bit for bit"""
    P.avgpool(ops, dt, N, 2048, 7, _record)


def test_softmax_and_ce_deriv_at_batch_256(ops):
    """256 x 1000 logits, with rows at |x| ~ 80-110 and rows of many equal maxima: soft-max against float64; ce_deriv = pred - onehot bit
    for bit (float32)"""
    P.softmax_ce(ops, N, 1000, _record)


def _decay(b, t):
    c = F(1)
    for _ in range(t):
        c = F(c * F(b))       # the trainer's float32 product (cur_mean_decay *= base_mean_decay)
    return c


@pytest.mark.parametrize("t,planted", [(1, False), (500, True)], ids=["t1", "t500_nan_inf"])
def test_adam_at_batch_256_arena(ops, t, planted):
    """Adam over an arena of ResNet-50's size (every tensor padded to 64 floats: > 2^24 elements) against the float64 formula from the
    same float32 inputs.  Planted: NaN / +-Inf gradients (the last element among them) keep m and v, and p is then formed from the kept
    moments (the reference's updateParams); an update that overflows keeps p; either sets the flag"""
    n = E.arena_floats(synth.R50_DIMS)
    rng = np.random.default_rng(80 + t)
    p = rng.standard_normal(n, dtype=F) * F(0.05)
    g = rng.standard_normal(n, dtype=F) * np.exp(rng.uniform(-8, 2, n)).astype(F)
    m = rng.standard_normal(n, dtype=F) * F(1e-2)
    v = np.abs(rng.standard_normal(n, dtype=F)) * F(1e-4)
    hp = dict(lr=1e-3, wd=5e-4, b1=0.9, b2=0.999, cb1=_decay(0.9, t), cb2=_decay(0.999, t), eps=1e-7)
    bad_g = np.array([0, 12345, 2 ** 24 + 7, n - 2, n - 1]) if planted else np.array([], int)
    ovf = np.array([99, n - 3]) if planted else np.array([], int)
    if planted:
        g[bad_g] = [np.nan, np.inf, -np.inf, np.nan, np.nan]
        m[ovf], v[ovf], g[ovf] = F(3e38), F(0), F(1)
    gp, gm, gv, flag = ops.adam(p, g, m, v, hp["lr"], hp["wd"], hp["b1"], hp["b2"], hp["cb1"], hp["cb2"], hp["eps"])
    assert flag == (1 if planted else 0)
    keep = np.zeros(n, bool)
    keep[ovf] = True
    assert np.array_equal(gp[ovf], p[ovf]), "an overflowing update must keep p"
    for i in range(0, n, 1 << 22):  # the float64 reference in blocks (host memory)
        sl = slice(i, i + (1 << 22))
        (rp, Ap), (rm, Am), (rv, Av) = E.adam_ref(p[sl], g[sl], m[sl], v[sl], **hp)
        ok = ~keep[sl]
        for name, got, ref, A, sel in (("p", gp[sl], rp, Ap, ok), ("m", gm[sl], rm, Am, slice(None)), ("v", gv[sl], rv, Av, slice(None))):
            w, bad = R.dist_f32(got[sel], ref[sel], A[sel])
            assert bad == 0, "Adam %s: %d out of bounds in [%d, %d) (worst %.3g)" % (name, bad, i, i + (1 << 22), w)
            _record(("adam t=%d" % t, name), w)
    assert np.array_equal(gm[bad_g], m[bad_g]) and np.array_equal(gv[bad_g], v[bad_g]), "a NaN / Inf gradient must keep m and v"
    assert np.all(np.isfinite(gp)), "p must stay finite"


def test_nhwc_to_nchw_at_batch_256(ops):
    P.nhwc_to_nchw(ops, N, 224)
