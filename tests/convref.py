"""Float64 reference of the convolutions on slabs of their outputs, and per-element checks against it (CPU only).

The reference is torch's CPU float64 convolution with the product's conventions (padding k // 2; the reference network's
projections are 3x3 stride 2, tests/torch_ref.py).  A full reference at batch 256 costs about a TMAC per operator, so it is
computed on slabs that cross every output tile of the kernels:
  * fwd / dgrad: every channel of a set S of images (0, N - 1, the images on both sides of the boundary between whole and
    sliced tiles that mi_conv_plan reports, and 3 seeded ones), and every image of a set R of channels (first and last of
    each 64-channel block plus 6 seeded ones per block);
  * wgrad: the rows R of K x all C * taps, and the columns R of C x all K * taps.

Error scale: A = the same operation on |operands| (+ |addend|), delta = C_FACTOR * 2^-24 * A.  In fp32 a sum of random-sign
terms is typically off by ~2^-24 A; one missing term costs ~A / n (n <= 18432 terms for fwd / dgrad).
  * fp32 outputs: |got - ref| <= delta
  * bf16 outputs: RNE(ref - delta) <= got <= RNE(ref + delta), RNE = round to the nearest bf16, ties to even
  * A == 0: got must be exactly 0
  * NaN is out of every bound
"""
import numpy as np
import torch
import torch.nn.functional as F

C_FACTOR = 64
U24 = 2.0 ** -24
CHUNK_BYTES = 2e9  # float64 working set per chunk of images


def set_threads(n=16):
    torch.set_num_threads(max(1, min(n, torch.get_num_threads())))


# ---------------------------------------------------------------------------------------------------------------------------
# bf16 rounding of float64 values, exactly (no detour through float32, which would round twice)
def rne_bf16(a):
    a = np.asarray(a, np.float64)
    m, e = np.frexp(a)                     # a = m * 2^e, 0.5 <= |m| < 1
    return np.ldexp(np.rint(m * 256.0), e - 8)  # 8 significant bits, np.rint rounds ties to even


def bf16_ulp(a):
    _, e = np.frexp(np.asarray(a, np.float64))
    return np.ldexp(1.0, e - 8)


def bf16_round32(a):
    """float32 -> the nearest bf16 value (ties to even), as float32"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# slabs
def slab_images(N, plan=None, M=None, P=None, seed=0):
    """S: 0, N-1, the images on both sides of the first sliced tile's first column (plan = mi_conv_plan's out, M = rows of the
    output matrix, P = pixels per image as the kernel counts them), 3 seeded ones"""
    s = {0, N - 1}
    if plan is not None and plan[3] < plan[2]:
        bm, bn, full = plan[0], plan[1], plan[3]
        col = (full // (M // bm)) * bn
        for c in (col - 1, col):
            if 0 <= c < N * P:
                s.add(c // P)
    rng = np.random.RandomState(1000 + seed)
    s.update(int(i) for i in rng.randint(0, N, 3))
    return sorted(s)


def slab_channels(Cn, seed=0):
    """R: first and last channel of every 64-channel block, 6 seeded ones per block"""
    rng = np.random.RandomState(2000 + seed)
    r = set()
    for b0 in range(0, Cn, 64):
        b1 = min(Cn, b0 + 64)
        r.update((b0, b1 - 1))
        r.update(int(i) for i in rng.choice(np.arange(b0, b1), min(6, b1 - b0), replace=False))
    return sorted(r)


# ---------------------------------------------------------------------------------------------------------------------------
# float64 operations (torch CPU); x, w, dy are numpy float32 / float64 arrays
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def fwd64(x, w, stride):
    k = w.shape[2]
    return F.conv2d(_t(x), _t(w), stride=stride, padding=k // 2).numpy()


def dgrad64(w, dy, H, stride):
    k = w.shape[2]
    Ho = dy.shape[2]
    op = H - ((Ho - 1) * stride - 2 * (k // 2) + k)
    return F.conv_transpose2d(_t(dy), _t(w), stride=stride, padding=k // 2, output_padding=op).numpy()


def wgrad64(x, dy, k, stride):
    K, Cn = dy.shape[1], x.shape[1]
    return torch.nn.grad.conv2d_weight(_t(x), (K, Cn, k, k), _t(dy), stride=stride, padding=k // 2).numpy()


def _chunk(N, per_image_floats):
    return max(1, min(N, int(CHUNK_BYTES / (8.0 * max(1, per_image_floats)))))


class Slab:
    """reference values `ref` and error scale `A` on one slab, with `take(got)` selecting the same elements from a full output"""

    def __init__(self, name, ref, A, take):
        self.name, self.ref, self.A, self.take = name, ref, A, take


def fwd_slabs(x, w, stride, S, R):
    N, Cn, H, _ = x.shape
    K, k = w.shape[0], w.shape[2]
    Ho = H // stride
    out = []
    xs = x[S]
    out.append(Slab("images %s" % (S,), fwd64(xs, w, stride), fwd64(np.abs(xs), np.abs(w), stride), lambda g, S=S: g[S]))
    wr, awr = w[R], np.abs(w[R])
    n = _chunk(N, 2 * (Cn * H * H + len(R) * Ho * Ho))
    ref = np.empty((N, len(R), Ho, Ho)); A = np.empty_like(ref)
    for i in range(0, N, n):
        ref[i:i + n] = fwd64(x[i:i + n], wr, stride)
        A[i:i + n] = fwd64(np.abs(x[i:i + n]), awr, stride)
    out.append(Slab("channels %d of %d" % (len(R), K), ref, A, lambda g, R=R: g[:, R]))
    return out


def dgrad_slabs(w, dy, H, stride, S, R, addend=None):
    N, K, Ho, _ = dy.shape
    Cn = w.shape[1]
    out = []
    ds = dy[S]
    ref, A = dgrad64(w, ds, H, stride), dgrad64(np.abs(w), np.abs(ds), H, stride)
    if addend is not None:
        ref += addend[S]; A += np.abs(addend[S])
    out.append(Slab("images %s" % (S,), ref, A, lambda g, S=S: g[S]))
    wr, awr = w[:, R], np.abs(w[:, R])
    n = _chunk(N, 2 * (K * Ho * Ho + len(R) * H * H))
    ref = np.empty((N, len(R), H, H)); A = np.empty_like(ref)
    for i in range(0, N, n):
        ref[i:i + n] = dgrad64(wr, dy[i:i + n], H, stride)
        A[i:i + n] = dgrad64(awr, np.abs(dy[i:i + n]), H, stride)
    if addend is not None:
        ref += addend[:, R]; A += np.abs(addend[:, R])
    out.append(Slab("channels %d of %d" % (len(R), Cn), ref, A, lambda g, R=R: g[:, R]))
    return out


def wgrad_slabs(x, dy, k, stride, RK, RC):
    """rows RK of K (all C * taps) and columns RC of C (all K * taps), each summed over every image"""
    N, Cn, H, _ = x.shape
    K, Ho = dy.shape[1], dy.shape[2]
    n = _chunk(N, 2 * (Cn * H * H + K * Ho * Ho))
    rows, rowsA = np.zeros((len(RK), Cn, k, k)), np.zeros((len(RK), Cn, k, k))
    cols, colsA = np.zeros((K, len(RC), k, k)), np.zeros((K, len(RC), k, k))
    for i in range(0, N, n):
        xc, dc = x[i:i + n], dy[i:i + n]
        ax, ad = np.abs(xc), np.abs(dc)
        rows += wgrad64(xc, dc[:, RK], k, stride); rowsA += wgrad64(ax, ad[:, RK], k, stride)
        if len(RC):
            cols += wgrad64(xc[:, RC], dc, k, stride); colsA += wgrad64(ax[:, RC], ad, k, stride)
    out = [Slab("rows %d of K" % len(RK), rows, rowsA, lambda g, RK=RK: g[RK])]
    if len(RC):
        out.append(Slab("columns %d of C" % len(RC), cols, colsA, lambda g, RC=RC: g[:, RC]))
    return out


def gate_slabs(slabs, mask):
    """the dgrad gated by mask > 0 (backwards_pass's ReLU'): ref and A are 0 where the gate is shut, so got must be exactly 0 there"""
    out = []
    for sl in slabs:
        on = sl.take(mask) > 0
        out.append(Slab(sl.name + " gated", np.where(on, sl.ref, 0.0), np.where(on, sl.A, 0.0), sl.take))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# reductions (batch-norm statistics and the BN' sums); bound C_FACTOR * 2^-24 * sum |terms| per channel
def bn_stats_ref(ref, A):
    """means and (biased) variances per channel of a convolution output known over every image (an R slab: [N, R, Ho, Ho]) and their
    bounds: the sum's own error plus what the convolution's per-element error (<= C_FACTOR 2^-24 A) carries into it"""
    ax = (0, 2, 3)
    mu = ref.mean(ax)
    d = ref - mu[None, :, None, None]
    var = (d * d).mean(ax)
    bm = C_FACTOR * U24 * (np.abs(ref) + A).mean(ax)
    bv = C_FACTOR * U24 * (ref * ref + 2 * np.abs(d) * A).mean(ax)
    return mu, var, bm, bv


def conv_stats_violations(gm, gv, ref, A):
    """channels of the kernel's (means, vars) [of the R slab's channels] outside the bounds of bn_stats_ref(ref, A), and the worst distance in
    2^-24 (bound scale) units"""
    mu, var, bm, bv = bn_stats_ref(ref, A)
    em, ev = np.abs(np.asarray(gm, np.float64) - mu), np.abs(np.asarray(gv, np.float64) - var)
    bad = int(np.count_nonzero(~(em <= bm))) + int(np.count_nonzero(~(ev <= bv)))
    return bad, float(max(np.max(em / bm), np.max(ev / bv))) * C_FACTOR


def bn_grad_sums(g, bn_x, means, vars_, eps):
    """float64 dbeta = sum g, dgamma = sum g (x - mean) / sqrt(var + eps) per channel of the product's own gated gradient g, with
    sum |terms| of each"""
    Cn = g.shape[1]
    inv = 1.0 / np.sqrt(vars_.astype(np.float64) + eps)
    db, dg, adb, adg = np.zeros(Cn), np.zeros(Cn), np.zeros(Cn), np.zeros(Cn)
    n = _chunk(g.shape[0], 3 * Cn * g.shape[2] * g.shape[3])
    for i in range(0, g.shape[0], n):
        gc = g[i:i + n].astype(np.float64)
        t = gc * ((bn_x[i:i + n] - means.astype(np.float64)[None, :, None, None]) * inv[None, :, None, None])
        db += gc.sum((0, 2, 3)); adb += np.abs(gc).sum((0, 2, 3))
        dg += t.sum((0, 2, 3)); adg += np.abs(t).sum((0, 2, 3))
    return db, dg, adb, adg


# ---------------------------------------------------------------------------------------------------------------------------
# per-element checks
def dist_f32(got, ref, A):
    """worst |got - ref| in units of 2^-24 A (inf where A == 0 and got != 0) and the number of elements out of bounds"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    pos = A > 0
    bad = int(np.count_nonzero(~(err[pos] <= C_FACTOR * U24 * A[pos]))) + int(np.count_nonzero(got[~pos] != 0))  # (NaN is out of bounds)
    worst = float(np.max(err[pos] / (U24 * A[pos]))) if pos.any() else 0.0
    if np.any(got[~pos] != 0) or np.isnan(worst):
        worst = float("inf")
    return worst, bad


def dist_bf16(got, ref, A):
    """worst |got - ref| as a fraction of a bf16 ulp of ref -- over the elements where d < ulp / 2, i.e. where the bound pins the
    rounding (elsewhere ref is small against A and either neighbour passes) -- and the number of elements outside
    [RNE(ref - d), RNE(ref + d)]"""
    got = np.asarray(got, np.float64)
    d = C_FACTOR * U24 * A
    lo, hi = rne_bf16(ref - d), rne_bf16(ref + d)
    pos = A > 0
    bad = int(np.count_nonzero(~((got >= lo) & (got <= hi))[pos])) + int(np.count_nonzero(got[~pos] != 0))
    ulp = bf16_ulp(ref)
    tight = pos & (d < 0.5 * ulp)
    worst = float(np.max(np.abs(got - ref)[tight] / ulp[tight])) if tight.any() else 0.0
    if np.any(got[~pos] != 0) or np.isnan(got[pos]).any():
        worst = float("inf")
    return worst, bad


def check_slabs(got, slabs, bf16, what):
    """every slab of `got` within its bounds; returns the worst distance (2^-24 A units, or bf16 ulps)"""
    worst = 0.0
    for s in slabs:
        g = s.take(got)
        w, bad = (dist_bf16 if bf16 else dist_f32)(g, s.ref, s.A)
        assert bad == 0, "%s, %s: %d elements out of bounds (worst %.3g %s)" % (what, s.name, bad, w, "bf16 ulp" if bf16 else "x 2^-24 A")
        worst = max(worst, w)
    return worst


def violations(got, slabs, bf16):
    """number of out-of-bound elements over all slabs (for the checker's own tests)"""
    return sum((dist_bf16 if bf16 else dist_f32)(s.take(got), s.ref, s.A)[1] for s in slabs)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference ResNet-50's convolutions at batch 256, as plan_layers (resnet_amd/csrc/trainer.c) lays them out: per bottleneck
# block a 1x1 reduction, a 3x3 spatial convolution with the block's stride, a 1x1 expansion, and in the first block of a stage the
# projection (3x3 stride 2; 1x1 where the stage keeps the plane).  (C, H, K, k, stride, where); "red" layers take the shortcut
# gradient as the addend of their dgrad (backwards_pass, red_addend).
N256 = 256
LAYERS = [
    (64, 56, 64, 1, 1, "b0 red"), (64, 56, 64, 3, 1, "stage 1 spa"), (64, 56, 256, 1, 1, "stage 1 exp, b0 proj"), (256, 56, 64, 1, 1, "stage 1 red"),
    (256, 56, 128, 1, 1, "b3 red"), (128, 56, 128, 3, 2, "b3 spa"), (128, 28, 512, 1, 1, "stage 2 exp"), (256, 56, 512, 3, 2, "b3 proj"),
    (512, 28, 128, 1, 1, "stage 2 red"), (128, 28, 128, 3, 1, "stage 2 spa"),
    (512, 28, 256, 1, 1, "b7 red"), (256, 28, 256, 3, 2, "b7 spa"), (256, 14, 1024, 1, 1, "stage 3 exp"), (512, 28, 1024, 3, 2, "b7 proj"),
    (1024, 14, 256, 1, 1, "stage 3 red"), (256, 14, 256, 3, 1, "stage 3 spa"),
    (1024, 14, 512, 1, 1, "b13 red"), (512, 14, 512, 3, 2, "b13 spa"), (512, 7, 2048, 1, 1, "stage 4 exp"), (1024, 14, 2048, 3, 2, "b13 proj"),
    (2048, 7, 512, 1, 1, "stage 4 red"), (512, 7, 512, 3, 1, "stage 4 spa"),
]
OPS = {"fwd": 0, "dgrad": 1, "wgrad": 2}
ROUTES = {"default": 0, "cl": 1, "cl2": 2, "pw": 3}


def conv_plan(L, dtype, route, op, N, Cn, H, K, k, s):
    """mi_conv_plan: (bm, bn, tiles, first sliced tile, slices, splits, grouped), or None where the route refuses the shape"""
    import ctypes
    out = (ctypes.c_int * 7)()
    rc = L.mi_conv_plan(dtype, ROUTES[route], OPS[op], N, Cn, H, K, k, s, out)
    return tuple(out) if rc == 0 else None


def layer_routes(L, dtype, policy, N, Cn, H, K, k, s, site=0):
    """mi_layer_routes: (fwd, dgrad, wgrad, fz) the library's planner -- the one its trainer and its operators run through -- gives a
    convolution under this process's switches (MI_FWD_* / MI_DG_* / MI_WG_*, include/resnet_mi.h), or None where it refuses"""
    import ctypes
    out = (ctypes.c_int * 4)()
    rc = L.mi_layer_routes(dtype, policy, N, Cn, H, K, k, s, site, out)
    return tuple(out) if rc == 0 else None


# the planner's bf16 routes in mi_conv_plan's route names, per op: MI_FWD_BF16 / MI_FWD_CL; MI_DG_BF16 / MI_DG_CL, MI_DG_CL2; MI_WG_BF16 /
# MI_WG_CL / MI_WG_CL2
BF16_ROUTE_NAMES = ({1: "default", 2: "cl"}, {1: "default", 2: "cl", 3: "cl"}, {1: "default", 2: "cl", 3: "cl2"})


def bf16_route(L, op, N, Cn, H, K, k, s):
    """the route the planner gives a bf16 layer (layer_routes).  Inside MI_WG_BF16 a 1x1 weight gradient takes the LDS-DMA kernel where
    that tiles (the planner's kernel choice, mi_layer_kernels), which mi_conv_plan's route "pw" answers"""
    r = layer_routes(L, 1, 0, N, Cn, H, K, k, s)
    assert r is not None, "the planner refuses the bf16 layer %s at N = %d" % ((Cn, H, K, k, s), N)
    name = BF16_ROUTE_NAMES[OPS[op]][r[OPS[op]]]
    if op == "wgrad" and name == "default" and k == 1 and conv_plan(L, 1, "pw", "wgrad", N, Cn, H, K, k, s) is not None:
        return "pw"
    return name


def blocks(dims):
    """the bottleneck blocks of a net (plan_layers' walk of init_dimensions' table): incoming / reduced / expanded channels, incoming plane,
    stride, and whether the block has a projection; with the stem's output plane Hs and filters f"""
    f, Hs = dims["init_conv_filters"], dims["input"] // dims["init_conv_stride"]
    out = []
    inc, red, ex, H = f, f, 4 * f, Hs // dims["init_maxpool_stride"]
    for i in range(dims["n_conv_blocks"]):
        s = 1
        if dims["is_block_spatial_reduction"][i]:
            s, red, ex = 2, red * 2, ex * 2
        out.append(dict(inc=inc, red=red, ex=ex, H=H, s=s, proj=inc != ex))
        inc, H = ex, H // s
    return out


def trainer_units(dims):
    """(block, role, (C, H, K, k, stride), site) of every bottleneck convolution in plan_layers order (per block: reduction, spatial,
    expansion, projection); site = its bit in the planner's BN'-fusion masks (mi_layer_plan): 4 the reduction of block i > 0 whose block below (i - 1) has no
    projection (its dgrad feeds that block's expansion BN'), 2 every spatial layer, 1 every expansion, 0 the projections"""
    bl = blocks(dims)
    out = []
    for i, b in enumerate(bl):
        H, s = b["H"], b["s"]
        out.append((i, "red", (b["inc"], H, b["red"], 1, 1), 4 if i > 0 and not bl[i - 1]["proj"] else 0))
        out.append((i, "spa", (b["red"], H, b["red"], 3, s), 2))
        out.append((i, "exp", (b["red"], H // s, b["ex"], 1, 1), 1))
        if b["proj"]:
            out.append((i, "proj", (b["inc"], H, b["ex"], 3 if s == 2 else 1, s), 0))
    return out


def trainer_layers(dims):
    """the distinct convolution shapes of a net in order of first appearance, (C, H, K, k, stride, where): where names each role the
    shape plays, "b<i> <role>" where one block has it, "stage <j> <role>" where several blocks of stage j do (stages 1, 2, ... begin at
    block 0 and at every striding block).  "red" in where: the dgrad takes the shortcut gradient as its addend (backwards_pass,
    red_addend, every block)"""
    bl = blocks(dims)
    stage, st = [], 0
    for b in bl:
        st += b["s"] == 2 or not stage
        stage.append(st)
    occ = {}
    for i, role, shape, _ in trainer_units(dims):
        occ.setdefault(shape, {}).setdefault(role, []).append(i)
    out = []
    for shape, roles in occ.items():
        tags = []
        for role, idx in roles.items():
            idx = sorted(set(idx))
            tags.append("b%d %s" % (idx[0], role) if len(idx) == 1 else "stage %d %s" % (stage[idx[0]], role))
        out.append(shape + (", ".join(tags),))
    return out


def trainer_sites(dims):
    """shape -> the set of BN'-fusion sites (trainer_units) its occurrences have"""
    out = {}
    for _, _, shape, site in trainer_units(dims):
        out.setdefault(shape, set()).add(site)
    return out


def trainer_conv_cases(L, dims, N):
    """(dtype, route, op, C, H, K, k, stride, where): every (layer, route) pair the trainer of this net at batch N gives in both storage
    types (bf16: the planner's routes, bf16_route), and the 1x1 forward on a channel-last input
    (mi_op_conv1x1_fwd_bf16_cl) at every 1x1 layer"""
    cases = []
    for (Cn, H, K, k, s, where) in trainer_layers(dims):
        for op in OPS:
            cases.append(("f32", "default", op, Cn, H, K, k, s, where))
            cases.append(("bf16", bf16_route(L, op, N, Cn, H, K, k, s), op, Cn, H, K, k, s, where))
        if k == 1:
            cases.append(("bf16", "pw", "fwd", Cn, H, K, k, s, where))
    return cases


def batch256_cases(L):
    """trainer_conv_cases of ResNet-50 at the benchmark's batch"""
    import synth
    return trainer_conv_cases(L, synth.R50_DIMS, N256)


# the stem (plan_layers: 7x7 stride 2, 3 -> 64 filters, 224 x 224): the fp32 trainer runs it exactly on the fp32 matrix cores
# (MI_FWD_STEM_F32 / MI_WG_STEM_F32), the bf16 one on the bf16 matrix cores (MI_FWD_STEM_BF16 / MI_WG_STEM_BF16); fp32 tensors either way
STEM = (3, 224, 64, 7, 2)


def trainer_conv_bn_cases(dims):
    """(dtype, C, H, K, k, stride, where): forward_pass pairs every convolution with its BN (mi_op_conv_bn_fwd_t: statistics from the
    convolution's epilogue; the bf16 layers on the NCHW kernels -- the channel-last ones are trainer_conv_bn_cl_cases)"""
    return [(dt,) + layer for layer in trainer_layers(dims) for dt in ("f32", "bf16")]


def trainer_conv_bn_cl_cases(L, dims, N):
    """(C, H, K, k, stride, where) of the bf16 layers whose forward takes the channel-last kernel at batch N (unit_fwd's MI_FWD_CL:
    mi_op_conv_bn_fwd_bf16_cl, statistics from that kernel's epilogue)"""
    return [layer for layer in trainer_layers(dims) if bf16_route(L, "fwd", N, *layer[:5]) == "cl"]


def trainer_dgrad_bn_cases(L, dims, N):
    """(dtype, C, H, K, k, stride, where) of the dgrads that also do the BN' reduction (the planner's fz, mi_layer_plan in layer.c) at batch N: fp32 the
    site-4 layers only (RESNET_MI_F32_BNFUSE_BWD = 4); bf16 every site (trainer_units) whose dgrad is on the NCHW kernels (bf16_route)"""
    sites = trainer_sites(dims)
    out = []
    for layer in trainer_layers(dims):
        st = sites[layer[:5]]
        if 4 in st:
            out.append(("f32",) + layer)
        if st & {1, 2, 4} and bf16_route(L, "dgrad", N, *layer[:5]) == "default":
            out.append(("bf16",) + layer)
    return out


def conv_bn_cases():
    """trainer_conv_bn_cases of ResNet-50"""
    import synth
    return trainer_conv_bn_cases(synth.R50_DIMS)


def dgrad_bn_cases(L):
    """trainer_dgrad_bn_cases of ResNet-50 at N = 256: site 4 = every "red" shape but b0's (it takes the shortcut addend), site 1 = every
    expansion dgrad; the spatial dgrads (site 2) of ResNet-50 all take the channel-last kernels there"""
    import synth
    return trainer_dgrad_bn_cases(L, synth.R50_DIMS, N256)


# the nets the per-element files check: (name, dims, N) -- ResNet-50 at the benchmark's batch and at a batch whose column counts are no
# multiple of any tile (33: every fwd / dgrad plan of the list has a partial last tile), the trajectory tests' nets at their batches
def nets():
    import synth
    return {"r50": synth.R50_DIMS, "c1s": synth.C1S_DIMS, "c4i": synth.C4I_DIMS}


def stem_shape(dims):
    """(C, H, K, k, stride) of the stem"""
    return (3, dims["input"], dims["init_conv_filters"], dims["init_kernel_dim"], dims["init_conv_stride"])
