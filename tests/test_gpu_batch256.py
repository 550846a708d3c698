"""Every convolution route of the reference ResNet-50 at the benchmark's batch (256), element by element against a float64 reference.

The kernel plans depend on N (tile heights, sliced tail rounds, split weight gradients and their grouped reduce): the operator tests at
N <= 16 never reach the plans the benchmark runs.  The case list is convref.batch256_cases: every (layer shape, route) pair plan_layers
gives the network in fp32 and in bf16 storage with default switches, plus the 1x1 forward on a channel-last input.  Each case is checked
per element on the slabs of convref (every channel of a few images, every image of a few channels per 64-channel block), to
64 * 2^-24 * A (A = the same sum over |terms|); bf16 outputs must lie between the RNE roundings of ref -/+ that bound.  The FC GEMM in
its three forms is checked in full.  The conv + BN pairs run on every route forward_pass takes: the implicit GEMM / bf16 NCHW kernels,
the channel-last 3x3 forward of the bf16 layers, and the stem in its three storage forms.  The bodies are tests/perelement.py's.
"""
import os

import pytest

import convref as R
import perelement as P

pytestmark = pytest.mark.gpu

N = R.N256
WORST = {}  # (dtype, route, op) -> worst distance, printed at the end of the module (bf16: where the bound pins the rounding)


def _record(key, worst):
    WORST[key] = max(WORST.get(key, 0.0), worst)


try:
    from resnet_amd import binding as _B
    _L = _B.load()
except RuntimeError:  # library not built: collection must still work; the tests then fail in the ops fixture
    _L = None
# an error in building the case lists fails collection loudly
CASES = R.batch256_cases(_L) if _L else []
CONV_BN_CL = R.trainer_conv_bn_cl_cases(_L, R.nets()["r50"], N) if _L else []
DGRAD_BN = R.dgrad_bn_cases(_L) if _L else []
CONV_BN = R.conv_bn_cases()
IDS = ["%s_%s_%s_C%d_H%d_K%d_k%d_s%d" % c[:8] for c in CASES]


@pytest.fixture(scope="module", autouse=True)
def _threads():
    R.set_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))
    yield
    print("\nworst distance per route at N = %d (fp32 and reductions: x 2^-24 A, bf16: bf16 ulps)" % N)
    for key in sorted(WORST):
        print("  %-4s %-9s %-20s %.3g" % (key + (WORST[key],)))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conv_route_at_batch_256(ops, case):
    P.conv_route(ops, case, N, _record)


@pytest.mark.parametrize("form", ["nn", "lt", "rt"])
def test_fc_gemm_at_batch_256(ops, form):
    """the FC layer's three products at 256 x 2048 x 1000: logits = X W, dW = X^T dY, dX = dY W^T (full float64 reference)"""
    P.fc_gemm(ops, form, N, 2048, 1000, _record)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("op", ["fwd", "wgrad"])
def test_stem_at_batch_256(ops, dt, op):
    """the 7x7 stride-2 stem on its matrix-core kernels (exact fp32, or bf16 operands with fp32 accumulation; fp32 tensors either way):
    the forward on the slabs, the weight gradient against the full float64 reduction over every image"""
    P.stem(ops, dt, op, N, R.STEM[1], _record)


def test_stem_wgrad_bf16_dy_at_batch_256(ops):
    """the bf16 trainer's stem weight gradient from its bf16 dY (mi_trainer_stem_dtype: st_wgrad_kernel<true>)"""
    P.stem(ops, "bf16", "wgrad", N, R.STEM[1], _record, dy_dt=P.BF16)


@pytest.mark.parametrize("case", CONV_BN, ids=["%s_C%d_H%d_K%d_k%d_s%d" % c[:6] for c in CONV_BN])
def test_conv_bn_fwd_at_batch_256(ops, case):
    """mi_op_conv_bn_fwd_t as forward_pass pairs a convolution with its BN: the BN statistics come from the convolution's epilogue
    (including the partial rows the sliced tail tiles write).  The convolution output is checked on the slabs; the means and variances
    of the channels in R against the float64 statistics of the exact convolution over all images, to C_FACTOR 2^-24 times the sum of
    |terms| plus what the convolution's own bound carries in (contract: statistics of the fp32 accumulators, before any rounding)"""
    P.conv_bn_fwd(ops, case, N, _record)


@pytest.mark.parametrize("layer", CONV_BN_CL, ids=["C%d_H%d_K%d_k%d_s%d" % c[:5] for c in CONV_BN_CL])
def test_conv_bn_fwd_channel_last_at_batch_256(ops, layer):
    """mi_op_conv_bn_fwd_bf16_cl: the bf16 3x3 layers as unit_fwd runs them (MI_FWD_CL), statistics from the channel-last kernel's epilogue"""
    P.conv_bn_fwd(ops, ("bf16",) + layer, N, _record, route="cl")


@pytest.mark.parametrize("variant", list(P.STEM_BN))
def test_stem_bn_fwd_at_batch_256(ops, variant):
    """mi_op_stem_bn_fwd_t: the stem + BN + ReLU with the statistics from the stem kernel's partials, in the fp32 trainer's form and the bf16
    trainer's two (convolution output fp32, or bf16 as it stores it by default)"""
    P.stem_bn_fwd(ops, variant, N, R.STEM[1], _record)


@pytest.mark.parametrize("case", DGRAD_BN, ids=["%s_C%d_H%d_K%d_k%d_s%d" % c[:6] for c in DGRAD_BN])
def test_dgrad_bn_bwd_at_fused_sites(ops, case):
    """mi_op_conv_dgrad_bn_bwd_{f32,bf16} at the trainer's BN'-fusion sites: the gated dgrad (mask > 0 ? dgrad (+ addend) : 0) on the
    slabs against the convolution reference; dbeta and dgamma against float64 sums of the product's own gated output as it is stored
    (the kernels' contract: kernels_igemm_bf16.hip sums the rounded gradient), to C_FACTOR 2^-24 sum |terms|"""
    P.dgrad_bn_bwd(ops, case, N, _record)
