"""Where every convolution route stops taking a batch, and what answers beyond it (CPU only: the planner is host code).

The limits are DESIGN.md's "Size limits" table, restated here in plain integers:
  fp32 implicit GEMM (igemm_kernel)        input and output tensor each fewer than 2^30 elements (32-bit byte offsets)
  bf16 NCHW kernels (bgemm_kernel)         each fewer than 2147480000 elements
  bf16 channel-last kernels                the same, and the padded channel-last operand below 4294000000 bytes
  every convolution                        fewer than 2^31 pixels per tensor (N * H * H)
For each ResNet-50 layer the largest accepted N is found by bisection and must be exactly where the limit puts it -- a guard that is
removed or moved fails here.  One batch further the answer is a refusal that names the size limit, or another route that is named:
never the same kernel.  The operators' entry points answer as the planner does, checked through their return codes (a refusal
precedes every allocation and launch, so it needs no GPU).

The helper of the GPU tests (tests/largeref.py) is pinned here too: the regeneration of any element from its flat index, the choice of
the slab images, the sparse form of the whole-batch statistics, and a host restatement of the direct kernel's former 32-bit offset
arithmetic as a mutant that the slab images of case (d) must catch.
"""
import ctypes

import numpy as np
import pytest

import convref as R
import ewref as E
import largeref as G
import synth

LIM_F32 = 1 << 30
LIM_BF16 = 2147480000
LIM_CL_BYTES = 4294000000
LIM_PIXELS = 1 << 31
FWD, DGRAD, WGRAD = 0, 1, 2
LAYER_IDS = ["C%d_H%d_K%d_k%d_s%d" % l[:5] for l in R.LAYERS]


@pytest.fixture(scope="module")
def L():
    from resnet_amd import binding
    lib = binding.load()
    lib.mi_clear_error()
    return lib


def n_below(limit, per_image):
    """the largest N with N * per_image < limit"""
    return (limit - 1) // per_image


def last_accepted(accepts, lo=256, hi=1 << 26):
    """bisection: the largest N in [lo, hi) that `accepts`, which holds at lo and fails at hi"""
    assert accepts(lo) and not accepts(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if accepts(mid):
            lo = mid
        else:
            hi = mid
    return lo


def igemm_takes(L, op, N, C, H, K, k, s):
    """mi_igemm_supported, as mi_debug_conv_plan reports it (out[0])"""
    out = (ctypes.c_int * 9)()
    L.mi_debug_conv_plan(op, N, C, H, K, k, s, out)
    return out[0] == 1


def tensors(C, H, K, s):
    return C * H * H, K * (H // s) * (H // s)


def error_of(L):
    e = L.mi_last_error().decode()
    L.mi_clear_error()
    return e


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer", R.LAYERS, ids=LAYER_IDS)
def test_fp32_implicit_gemm_boundary(L, layer):
    """igemm_kernel takes a layer up to the last N at which both tensors hold fewer than 2^30 elements; one further mi_conv_plan answers
    "not this kernel", the planner keeps MI_*_F32 (the older kernels, which address with 64 bits or per image) and the operator agrees;
    at 2^31 pixels the planner refuses and names the limit"""
    C, H, K, k, s, _ = layer
    want = n_below(LIM_F32, max(tensors(C, H, K, s)))
    for op in (FWD, DGRAD, WGRAD):
        if not igemm_takes(L, op, R.N256, C, H, K, k, s):
            continue
        got = last_accepted(lambda n: igemm_takes(L, op, n, C, H, K, k, s))
        assert got == want, "op %d: the implicit GEMM takes N <= %d, the 2^30-element limit says %d" % (op, got, want)
        name = {FWD: "fwd", DGRAD: "dgrad", WGRAD: "wgrad"}[op]
        assert R.conv_plan(L, 0, "default", name, want, C, H, K, k, s) is not None
        for n in (want + 1, 2 * want, 4 * want + 3):
            assert R.conv_plan(L, 0, "default", name, n, C, H, K, k, s) is None, "mi_conv_plan still plans the implicit GEMM at N = %d" % n
    npix = n_below(LIM_PIXELS, H * H)
    assert R.layer_routes(L, 0, 0, want + 1, C, H, K, k, s) == (0, 0, 0, 0)
    assert R.layer_routes(L, 0, 0, npix, C, H, K, k, s) == (0, 0, 0, 0), error_of(L)
    assert error_of(L) == ""
    assert R.layer_routes(L, 0, 0, npix + 1, C, H, K, k, s) is None
    assert "size limit" in error_of(L) and error_of(L) == ""


@pytest.mark.parametrize("layer", R.LAYERS, ids=LAYER_IDS)
def test_bf16_nchw_boundary(L, layer):
    """bgemm_kernel (mi_bf16_conv_supported, mi_conv_plan's bf16 default route) up to the last N with both tensors below 2147480000
    elements; beyond it the planner has no bf16 route: mi_layer_routes refuses and names the limit"""
    C, H, K, k, s, _ = layer
    want = n_below(LIM_BF16, max(tensors(C, H, K, s)))
    for op, name in ((FWD, "fwd"), (DGRAD, "dgrad"), (WGRAD, "wgrad")):
        got = last_accepted(lambda n: L.mi_bf16_conv_supported(op, n, C, H, K, k, s) == 1)
        assert got == want, "op %d: the bf16 NCHW kernels take N <= %d, the limit says %d" % (op, got, want)
        assert R.conv_plan(L, 1, "default", name, want, C, H, K, k, s) is not None
        assert R.conv_plan(L, 1, "default", name, want + 1, C, H, K, k, s) is None
    assert R.layer_routes(L, 1, 0, want, C, H, K, k, s) is not None and error_of(L) == ""
    for n in (want + 1, 2 * want):
        assert R.layer_routes(L, 1, 0, n, C, H, K, k, s) is None
        assert "size limit" in error_of(L)


def _cl_fwd_limit(C, H, K, s):
    tin, tout = tensors(C, H, K, s)
    plane = 4 * (H // 2 + 1) ** 2 if s == 2 else (H + 2) ** 2
    return min(n_below(LIM_CL_BYTES, plane * C * 2), n_below(LIM_BF16, tin), n_below(LIM_BF16, tout))


@pytest.mark.parametrize("layer", [l for l in R.LAYERS if l[3] == 3], ids=[i for i, l in zip(LAYER_IDS, R.LAYERS) if l[3] == 3])
def test_bf16_channel_last_boundary(L, layer):
    """the channel-last 3x3 forward up to the last N whose padded operand stays below 4294000000 bytes (and both tensors below
    2147480000 elements); one further the planner names another route, the NCHW kernels, which take the layer until their own limit"""
    C, H, K, k, s, _ = layer
    want = _cl_fwd_limit(C, H, K, s)
    got = last_accepted(lambda n: R.conv_plan(L, 1, "cl", "fwd", n, C, H, K, k, s) is not None)
    assert got == want, "the channel-last forward takes N <= %d, the limits say %d" % (got, want)
    at, past = R.layer_routes(L, 1, 0, want, C, H, K, k, s), R.layer_routes(L, 1, 0, want + 1, C, H, K, k, s)
    assert at is not None and at[0] == 2, "MI_FWD_CL at the last accepted batch: %s" % (at,)
    nchw = n_below(LIM_BF16, max(tensors(C, H, K, s)))
    if want < nchw:
        assert past is not None and past[0] == 1 and past[2] == 1, "one batch further: MI_FWD_BF16 / MI_WG_BF16, not %s" % (past,)
    else:
        assert past is None and "size limit" in error_of(L)
    assert error_of(L) == ""
    if s == 2:  # the stride-2 dgrad on the channel-last dY: its own operand and the input tensor
        want2 = min(n_below(LIM_CL_BYTES, (H // 2 + 1) ** 2 * K * 2), n_below(LIM_BF16, C * H * H))
        took = lambda n: (R.layer_routes(L, 1, 0, n, C, H, K, k, s) or (0, 0))[1] == 3
        if took(R.N256):
            assert last_accepted(took) == want2
            error_of(L)


OPS_BF16 = (("mi_op_conv_fwd_bf16", FWD), ("mi_op_conv_dgrad_bf16", DGRAD), ("mi_op_conv_wgrad_bf16", WGRAD))


@pytest.mark.parametrize("layer", [R.LAYERS[3], R.LAYERS[1], R.LAYERS[7]], ids=[LAYER_IDS[3], LAYER_IDS[1], LAYER_IDS[7]])
def test_operators_refuse_where_the_planner_does(L, layer):
    """mi_op_conv_*_bf16 (and the forced channel-last forward) one batch past the route's limit: -2 before anything is allocated or
    launched (no device is needed: the pointers are never touched), mi_last_error names the size limit.  fp32: the operators take every
    batch the planner takes, so they refuse only at the pixel limit"""
    C, H, K, k, s, _ = layer
    n = n_below(LIM_BF16, max(tensors(C, H, K, s))) + 1
    for fn, op in OPS_BF16:
        extra = (0,) if op == DGRAD else ()
        assert getattr(L, fn)(None, None, None, n, C, H, K, k, s, *extra) == -2, fn
        assert "size limit" in error_of(L), fn
    if k == 3:
        assert L.mi_op_conv_fwd_bf16_cl(None, None, None, _cl_fwd_limit(C, H, K, s) + 1, C, H, K, s) == -2
        assert "size limit" in error_of(L)
    npix = n_below(LIM_PIXELS, H * H) + 1
    assert L.mi_op_conv_fwd(None, None, None, npix, C, H, K, k, s) == -2 and "size limit" in error_of(L)
    assert L.mi_op_conv_dgrad(None, None, None, npix, C, H, K, k, s, 0) == -2 and "size limit" in error_of(L)
    assert L.mi_op_conv_wgrad(None, None, None, npix, C, H, K, k, s) == -2 and "size limit" in error_of(L)
    assert L.mi_op_conv_dgrad_bn_bwd_f32(None, None, None, None, npix, C, H, K, k, s, None, None, None, None, None, None, 1e-7, None, None, None) == -2
    assert "size limit" in error_of(L)


def test_stem_refuses_at_the_pixel_limit(L):
    C, H, K, k, s = R.STEM
    npix = n_below(LIM_PIXELS, H * H)
    for dt in (0, 1):
        assert R.layer_routes(L, dt, 0, npix, C, H, K, k, s) is not None and error_of(L) == ""
        assert R.layer_routes(L, dt, 0, npix + 1, C, H, K, k, s) is None and "size limit" in error_of(L)
    assert L.mi_op_stem_fwd_f32(None, None, None, npix + 1, H) == -2 and "size limit" in error_of(L)


def test_the_cases_of_the_gpu_tests_are_where_the_issue_puts_them(L):
    """the batches tests/test_gpu_large.py derives: the top of each accepted range and the first batch past the fp32 limit"""
    assert last_accepted(lambda n: igemm_takes(L, FWD, n, 256, 56, 64, 1, 1)) == 1337
    assert last_accepted(lambda n: igemm_takes(L, FWD, n, 64, 56, 64, 3, 1)) == 5349
    assert last_accepted(lambda n: L.mi_bf16_conv_supported(FWD, n, 256, 56, 64, 1, 1) == 1) == 2674
    # three whole images past the one that holds byte 2^31: 672 at 802816 floats per image; 2678 at 200704 floats or 401408 bf16 (the GPU
    # cases take 2680 there) and 1341 at 802816 bf16 (they take 1344)
    assert G.smallest_crossing_n(802816, 4) == 672 and G.smallest_crossing_n(200704, 4) == 2678
    assert G.smallest_crossing_n(401408, 2) == 2678 and G.smallest_crossing_n(802816, 2) == 1341


# ---------------------------------------------------------------------------------------------------------------------------
# tests/largeref.py
def _fill_scalar(seed, i, lo, hi):
    """fill_uniform_kernel (kernels_misc.hip) for one element, in Python integers and doubles"""
    m = (1 << 64) - 1
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z ^= z >> 31
    u = float(z >> 11) * (1.0 / 9007199254740992.0)
    return np.float32(float(np.float32(lo)) + (float(np.float32(hi)) - float(np.float32(lo))) * u)


@pytest.mark.parametrize("start", [0, 12345, (1 << 29) - 3, (1 << 30) - 2, (1 << 31) - 1, (1 << 32) - 5, (1 << 33) + 7])
def test_regen_rebuilds_any_run_of_the_stream(start):
    got = G.regen(77, -1.0, 1.0, start, 64)
    want = np.array([_fill_scalar(77, start + i, -1.0, 1.0) for i in range(64)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if start < (1 << 20):
        whole = synth.uniform(77, start + 64, -1.0, 1.0)
        assert np.array_equal(got, whole[start:])
    bf = G.regen(77, -1.0, 1.0, start, 64, G.BF16)
    assert np.array_equal(bf, R.bf16_round32(want)) and np.all((bf.view(np.uint32) & 0xFFFF) == 0)


def test_regen_images_and_the_host_limit():
    imgs = G.regen_images(5, -2.0, 3.0, [0, 3, 700], 1000)
    assert imgs.shape == (3, 1000) and np.array_equal(imgs[2], G.regen(5, -2.0, 3.0, 700 * 1000, 1000))
    with pytest.raises(AssertionError):
        G.regen(5, 0.0, 1.0, 0, (G.HOST_LIMIT // 4) + 1)


def test_boundary_images():
    """0, N - 1, the image with the element at byte 2^31 (2^32 where reached) and its neighbours, two seeded; three whole images past it"""
    E_, N = 802816, 672
    S = G.boundary_images(N, E_, 4, seed=1)
    n31 = (1 << 31) // (E_ * 4)
    assert n31 * E_ * 4 <= (1 << 31) < (n31 + 1) * E_ * 4
    assert {0, N - 1, n31 - 1, n31, n31 + 1} <= set(S) and len(S) <= 7 and S == sorted(set(S))
    assert N - 1 - n31 == 3
    with pytest.raises(AssertionError):
        G.boundary_images(N - 1, E_, 4)
    S = G.boundary_images(1338, E_, 4, need_past=0)
    n32 = (1 << 32) // (E_ * 4)
    assert n32 == 1337 and {n32 - 1, n32, n31, 0} <= set(S) and max(S) == 1337
    assert G.boundary_images(100, 1000, 4) == sorted(set(G.boundary_images(100, 1000, 4))) and len(G.boundary_images(100, 1000, 4)) <= 4
    for E2, item in ((200704, 4), (401408, 2), (802816, 2)):
        n = G.smallest_crossing_n(E2, item)
        G.boundary_images(n, E2, item)
        with pytest.raises(AssertionError):
            G.boundary_images(n - 1, E2, item)


def test_sparse_statistics_are_the_dense_ones_with_zero_images():
    """sparse_stats_ref / sparse_bn_stats against convref.bn_stats_ref / ewref.stats_ref on a small batch whose other images are zero"""
    rng = np.random.default_rng(3)
    N, S = 11, [0, 4, 10]
    ref = np.zeros((N, 5, 6, 6)); A = np.zeros_like(ref)
    ref[S] = rng.standard_normal((3, 5, 6, 6)) + 0.4
    A[S] = np.abs(rng.standard_normal((3, 5, 6, 6))) + 1.0
    dense = R.bn_stats_ref(ref, A)
    sparse = G.sparse_stats_ref(ref[S], A[S], N * 36)
    for a, b in zip(dense, sparse):
        assert np.allclose(a, b, rtol=1e-12, atol=0)
    x = ref.astype(np.float32)
    for a, b in zip(E.stats_ref(x), G.sparse_bn_stats(x[S], N * 36)):
        assert np.allclose(a, b, rtol=1e-12, atol=0)
    bad, w = G.stats_distance(dense[0], dense[1], sparse)
    assert bad == 0 and w < 1e-3
    bad, _ = G.stats_distance(dense[0] * (1 + 1e-4), dense[1], sparse)
    assert bad > 0


# ---------------------------------------------------------------------------------------------------------------------------
# the direct kernel's former offset arithmetic as a mutant
def _dconv_row_offset_32(n, c, ih, Cin, Hin, Win):
    """dconv_kernel before the fix: the row table entry (int)((n * Cin * Hin + ih) * Win) of channel 0's row in 32 bits (negative = treated
    as padding), the byte offset (uint32_t)(t + iw) * 4 added to the channel's 64-bit base.  Returns the flat element the load of iw = 0
    lands on, or None (read as zero)"""
    t = ((n * Cin * Hin + ih) * Win) & 0xFFFFFFFF
    if t >= 1 << 31:
        return None
    return ((t * 4) & 0xFFFFFFFF) // 4 + c * Hin * Win


def _mutant_on_slabs(N, Cin, H):
    S = G.boundary_images(N, Cin * H * H, 4, need_past=0)
    wrong = zero = 0
    for n in S:
        for c in (0, Cin - 1):
            for ih in (0, H - 1):
                got = _dconv_row_offset_32(n, c, ih, Cin, H, H)
                zero += got is None
                wrong += got is not None and got != ((n * Cin + c) * H + ih) * H
    return S, wrong, zero


def test_the_former_direct_kernel_offsets_wrap_where_the_slab_images_look():
    """3x3 64 -> 64 @56 on the direct kernel.  The 32-bit part of its former offset was the row of CHANNEL 0 of the image (the channel went
    into the 64-bit base), so at the first batch the implicit GEMM declines (5350: the last image starts below 2^30 elements) it was
    still right; from image 5350 on the rows came from 2^32 bytes lower, from image 10700 on they were read as zeros.  The slab images
    of the GPU cases past the limit (N = 5353) hold such rows; with per-workgroup 64-bit image bases every row lands on its own element"""
    Cin, H = 64, 56
    first = (LIM_F32 - 1) // (Cin * H * H) + 1
    assert first == 5350
    assert _mutant_on_slabs(first, Cin, H)[1:] == (0, 0)
    S, wrong, zero = _mutant_on_slabs(first + 3, Cin, H)
    assert wrong > 0 and zero == 0, "the mutant must be caught on the slab images %s" % (S,)
    assert {first, first + 2} <= set(S)
    S, wrong, zero = _mutant_on_slabs(2 * first + 3, Cin, H)
    assert wrong > 0 and zero > 0
    assert _dconv_row_offset_32(first, 0, 0, Cin, H, H) == first * Cin * H * H - LIM_F32 == 24576, "image 5350 read from image 0"
