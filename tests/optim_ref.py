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


def step(kind, ws, gs, bs, is_weight, lr, wd, momentum, tau=0.001):
    """one update; returns (ws, gs, bs, flag) as float64 lists"""
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
