"""float64 numpy model of gradient clipping by the global L2 norm (include/resnet_mi.h, "gradient clipping"; kernels_optim.hip) and of
momentum SGD with two weight-decay groups (mi_trainer_set_norm_weight_decay).  tests/test_clip_model.py pins both against torch on the CPU.

  norm    sum g^2 per chunk of at most optim_ref.CHUNK floats (chunks never cross a tensor) and in total, in float64
  coef    norm = sqrt(sq); coef = min(1, max_norm / (norm + 1e-6)) in float64, rounded to float32 ONCE
          sq NaN or Inf: coef = 1, nonfinite = 1 -- the gradient is left to the optimizers' guards (torch.nn.utils.clip_grad_norm_ would
          make every gradient NaN: the documented departure)
  scale   float32(g) * float32(coef), one float32 product per element; coef == 1: the words of g as they are (-0, denormals, NaN payloads)

`fault`: one of FAULTS, a planted fault of the three kernels restated on the kernels' walk -- quad q of a chunk is thread q % 256's, its
turn q // 256; partial c of the coefficient pass is lane c % 64's, its turn c // 64 (the CPU pre-check of the GPU operator test).
"""
import numpy as np

import optim_ref as R

CHUNK = R.CHUNK
FAULTS = ("norm_whole_last_quad",       # the last quad per thread of a whole chunk left out of the norm
          "coef_second_lane_turn",      # the partials a lane reaches after its first turn (chunk 64 and up) left out
          "scale_tail_unscaled")        # the scalar tail behind the float4 body of a chunk left unscaled


def _f32(g):
    g = np.ascontiguousarray(g).ravel()
    return g.view(np.float32) if g.dtype == np.uint32 else g.astype(np.float32, copy=False)


def chunk_sq(gs, fault=None):
    """sum g^2 of every chunk of every tensor, in the chunk table's order, float64"""
    out = []
    for g in gs:
        g = _f32(g).astype(np.float64)
        for s in range(0, g.size, CHUNK):
            c = g[s:s + CHUNK]
            if fault == "norm_whole_last_quad" and c.size == CHUNK:
                c = c[(np.arange(CHUNK) // 4) // 256 != CHUNK // 4 // 256 - 1]
            with np.errstate(all="ignore"):
                out.append(np.sum(c * c))
    return np.array(out, np.float64)


def coefficient(sq, max_norm):
    """(coef as float32, norm, nonfinite) from the squared norm; max_norm is the float32 the kernel is handed"""
    max_norm = np.float64(np.float32(max_norm))
    if not np.isfinite(sq):
        with np.errstate(all="ignore"):
            return np.float32(1.0), np.sqrt(sq), 1
    norm = np.sqrt(np.float64(sq))
    r = max_norm / (norm + 1e-6)
    return (np.float32(r) if r < 1.0 else np.float32(1.0)), norm, 0


def scale(g, coef, fault=None):
    """float32(g) * float32(coef) per element; coef == 1: g's words untouched"""
    g = _f32(g)
    coef = np.float32(coef)
    if coef == np.float32(1.0):
        return g.copy()
    with np.errstate(all="ignore"):
        out = (g * coef).astype(np.float32)
    if fault == "scale_tail_unscaled":
        for s in range(0, g.size, CHUNK):
            n = min(CHUNK, g.size - s)
            out[s + n // 4 * 4:s + n] = g[s + n // 4 * 4:s + n]
    return out


def clip(gs, max_norm, fault=None):
    """the three passes over the tensors gs: (scaled tensors as float32, record) with record = dict(sq_norm, norm, coef, nonfinite,
    clipped) -- sq_norm and norm are those BEFORE the scaling, what torch's clip_grad_norm_ returns"""
    part = chunk_sq(gs, fault)
    if fault == "coef_second_lane_turn":
        part = part[:64]
    with np.errstate(all="ignore"):
        sq = np.sum(part)
    coef, norm, bad = coefficient(sq, max_norm)
    rec = dict(sq_norm=float(sq), norm=float(norm), coef=coef, nonfinite=bad, clipped=int(coef < np.float32(1.0)))
    return [scale(g, coef, fault) for g in gs], rec


def sgd_two_groups(ws, gs, bs, is_weight, lr, wd, wd_norm, momentum):
    """momentum SGD with two decay groups -- the tensors with is_weight 1 decay with wd, the others with wd_norm -- composed from
    optim_ref.step, one call per group; returns (ws, gs, bs, flag) as optim_ref.step does, the flag naming the highest offending tensor
    of the whole list"""
    n = len(ws)
    out = [[None] * n for _ in range(3)]
    flag = 0
    for decay, members in ((wd, [i for i in range(n) if is_weight[i]]), (wd_norm, [i for i in range(n) if not is_weight[i]])):
        if not members:
            continue
        w, g, b, f = R.step(R.SGD, [ws[i] for i in members], [gs[i] for i in members], [bs[i] for i in members], [1] * len(members), lr,
                            decay, momentum)
        for j, i in enumerate(members):
            out[0][i], out[1][i], out[2][i] = w[j], g[j], b[j]
        if f:
            flag = max(flag, members[f - 1] + 1)
    return out[0], out[1], out[2], flag


# ---- the inputs of tests/test_gpu_clip.py's operator test, shared with the CPU pre-check ----
# optim_ref.LOOP_TURN_SIZES (a vector, one half chunk, 66 chunks, one partial chunk of 513 quads: three turns of the float4 loop), then
# exactly one whole chunk, then 4 x 300 + 3 floats: a partial chunk that ends in three scalars.  71 chunks: seven lanes of the coefficient
# pass take a second turn.  Only the last tensor's length may be no multiple of 4 (offsets are multiples of 4)
OP_SIZES = R.LOOP_TURN_SIZES + [CHUNK, 4 * 300 + 3]
OP_OFFSETS = [sum(OP_SIZES[:i]) for i in range(len(OP_SIZES) + 1)]
# magnitudes 1e-4 .. 1e2 across the tensors, fixed so that the whole chunks (tensors 2 and 4) and the chunks from 64 on carry a share of
# the squared norm far above the test's 1e-12
OP_MAGNITUDES = [1e2, 1e-4, 1e-2, 1.0, 1e-1, 1e1]
# test (a): sq_norm to 1e-12 relative (the order of the float64 sums differs), coef within one float32 ulp, elements bit for bit
OP_SQ_REL = 1e-12


def op_gradient(seed=7):
    """the operator test's gradient as one float32 array over OP_OFFSETS"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.standard_normal(n, dtype=np.float32) * np.float32(m) for n, m in zip(OP_SIZES, OP_MAGNITUDES)])


def split(a, offs):
    return [a[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def ulps32(a, b):
    """distance of two positive float32 numbers in units in the last place"""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))
