"""float64 numpy model of the momentum SGD and LARS rules of update_parameters (include/resnet_mi.h, kernels_optim.hip),
guards included.

A step takes the per-tensor lists w, g, b (any float dtype; computed in float64) and returns the new lists and the NaN flag:

  SGD    d = g + wd w;  b = mu b + d;  w = w - lr b                                   (torch.optim.SGD, dampening 0, no Nesterov)
  LARS   weights:  trust = tau |w| / (|g| + wd |w|) where |w| > 0 and |g| > 0, else 1;  b = mu b + lr trust (g + wd w);  w = w - b
         BN gamma / beta:  b = mu b + lr g;  w = w - b
         the norms per tensor, over the whole tensor, before any update

Guards (the contract of the Adam kernel):
  * an element whose gradient is NaN / Inf keeps its w and b, and the gradient stays; finite gradients are cleared
  * an element whose new w or b is not finite keeps both
  * LARS: a tensor with a norm that is not finite (a NaN / Inf in its w or g) keeps all of its w and b.  SGD has no norm pass:
    there the guard is the per-element one
  * the flag is the highest offending tensor index + 1 (0: clean)
"""
import numpy as np

SGD, LARS = 1, 2


def sq_norms(ws, gs):
    """per tensor (sum w^2, sum g^2) in float64"""
    return np.array([[np.sum(np.square(np.asarray(w, np.float64))), np.sum(np.square(np.asarray(g, np.float64)))]
                     for w, g in zip(ws, gs)])


def trust_ratio(sw, sg, wd, tau):
    """LARS trust ratio of a weight tensor from its squared norms (1 where a norm is zero)"""
    wn, gn = np.sqrt(sw), np.sqrt(sg)
    if wn > 0 and gn > 0:
        return tau * wn / (gn + wd * wn)
    return 1.0


def _fault_masks(size, fault):
    """per element of a tensor: (left out of sum w^2, left out of sum g^2, runs without weight decay, momentum read as 0) under `fault`,
    from the kernels' walk: chunk c holds floats [c CHUNK, ...); quad q of a chunk is thread q % 256's, its turn q // 256"""
    no_w, no_g, no_wd, no_b = (np.zeros(size, bool) for _ in range(4))
    for ci, s in enumerate(range(0, size, CHUNK)):
        n = min(CHUNK, size - s)
        n4 = n // 4
        quad = np.arange(n) // 4
        body = np.arange(n) < 4 * n4
        whole = n4 == CHUNK // 4
        sl = slice(s, s + n)
        if fault == "norm_whole_last_quad" and whole:
            no_g[sl] = quad // 256 == CHUNK // 4 // 256 - 1
        elif fault == "norm_partial_second_turn" and not whole:
            no_w[sl] = no_g[sl] = body & (quad >= 256)
        elif fault == "norm_wave3":
            thread = np.where(body, quad % 256, np.arange(n) - 4 * n4)
            no_w[sl] = no_g[sl] = thread >= 192
        elif fault == "trust_second_lane_turn" and ci >= 64:
            no_w[sl] = no_g[sl] = True
        elif fault == "update_whole_last_w_no_decay" and whole:
            no_wd[sl] = (quad // 256 == CHUNK // 4 // 256 - 1) & (np.arange(n) % 4 == 3)
        elif fault == "update_partial_second_turn_no_momentum" and not whole:
            no_b[sl] = body & (quad >= 256)
    return no_w, no_g, no_wd, no_b


def _faulty_step(kind, ws, gs, bs, is_weight, lr, wd, mu, tau, fault):
    """step() with one planted fault of the optimizer kernels restated (no non-finite values: the guards are not modelled here)"""
    out_w, out_g, out_b = [], [], []
    for i, (w, g, b) in enumerate(zip(ws, gs, bs)):
        w, g, b = (np.array(a, np.float64).ravel() for a in (w, g, b))
        no_w, no_g, no_wd, no_b = _fault_masks(w.size, fault)
        wde = np.where(no_wd, 0.0, wd)
        be = np.where(no_b, 0.0, b)
        if kind == SGD:
            nb = mu * be + (g + wde * w)
            nw = w - lr * nb
        else:
            if is_weight[i]:
                wn, gn = np.sqrt(np.sum(np.square(w[~no_w]))), np.sqrt(np.sum(np.square(g[~no_g])))
                ok = gn > 0 if fault == "guard_gn_only" else (wn > 0 and gn > 0)
                t = tau * wn / (gn + wd * wn) if ok else 1.0
                nb = mu * be + lr * t * (g + wde * w)
            else:
                nb = mu * be + lr * g
            nw = w - nb
        out_w.append(nw); out_b.append(nb); out_g.append(np.zeros_like(g))
    return out_w, out_g, out_b, 0


CHUNK = 8192   # MID_OPT_CHUNK: floats per workgroup of the norm and update passes; 256 threads, one float4 each per turn
# tensors of test_gpu_optim.py::test_lars_loop_turns_and_an_all_zero_weight_tensor: a BN vector, an all-zero weight tensor, a weight tensor
# of 66 chunks (a second lane turn of the trust kernel), a weight tensor that is one partial chunk of 513 quads (three turns of its float4 loops)
LOOP_TURN_SIZES = [64, 4096, 65 * CHUNK + 4, 1024 + 256 * 4 + 4]
LOOP_TURN_OFFSETS = [sum(LOOP_TURN_SIZES[:i]) for i in range(len(LOOP_TURN_SIZES) + 1)]
LOOP_TURN_IS_WEIGHT = [0, 1, 1, 1]


def chunks_of(size):
    """the lengths of the chunks a tensor of `size` floats is cut into"""
    return [min(CHUNK, size - s) for s in range(0, size, CHUNK)]


def step(kind, ws, gs, bs, is_weight, lr, wd, momentum, tau=0.001, fault=None):
    """one update; returns (ws, gs, bs, flag) as float64 lists.  fault: one of the planted faults of tests/mutants.py restated (the CPU
    pre-checks of tests/test_loop_turns_model.py): "guard_gn_only", "trust_second_lane_turn", "norm_whole_last_quad",
    "norm_partial_second_turn", "norm_wave3", "update_whole_last_w_no_decay", "update_partial_second_turn_no_momentum" """
    if fault:
        return _faulty_step(kind, ws, gs, bs, is_weight, lr, wd, momentum, tau, fault)
    lr, wd, mu, tau = float(lr), float(wd), float(momentum), float(tau)
    out_w, out_g, out_b, flag = [], [], [], 0
    sq = sq_norms(ws, gs) if kind == LARS else None
    for i, (w, g, b) in enumerate(zip(ws, gs, bs)):
        w, g, b = (np.array(a, np.float64).ravel() for a in (w, g, b))
        ok = np.isfinite(g)
        skip = False
        if kind == SGD:
            d = g + wd * w
            nb = mu * b + d
            nw = w - lr * nb
        elif kind == LARS:
            skip = not (np.isfinite(sq[i, 0]) and np.isfinite(sq[i, 1]))
            if is_weight[i]:
                t = 1.0 if skip else trust_ratio(sq[i, 0], sq[i, 1], wd, tau)
                nb = mu * b + lr * t * (g + wd * w)
            else:
                nb = mu * b + lr * g
            nw = w - nb
        else:
            raise ValueError(kind)
        with np.errstate(invalid="ignore", over="ignore"):
            take = ok & np.isfinite(nb) & np.isfinite(nw) & (not skip)
        bad = skip or not take[ok].all() or not ok.all()
        if bad:
            flag = i + 1
        out_w.append(np.where(take, nw, w))
        out_b.append(np.where(take, nb, b))
        out_g.append(np.where(ok, 0.0, g))
    return out_w, out_g, out_b, flag
