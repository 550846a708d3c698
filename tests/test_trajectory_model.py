"""CPU checks of what tests/test_gpu_trajectory.py measures the product against: the float64 Adam of torch_ref against the oracle's,
over several steps, and the committed ResNet-50 model loss curves (tools/trajectory_curves.py) against a recomputation."""
import os
import sys

import numpy as np
import pytest

import synth
import torch_ref
from util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "trajectory_r50_b8.npz")


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_model_matches_the_oracle_over_25_steps(oracle, wd):
    """decays advance before use (step t divides by 1 - beta^t), beyond the two steps the whole-step tests reach; a NaN / Inf
    gradient leaves the moments alone"""
    h = {k: float(np.float32(v)) for k, v in dict(lr=1e-4, wd=wd, b1=0.9, b2=0.999, eps=1e-7).items()}
    n = 4096
    p = synth.normal(11, n, 1.0)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    mp, mm, mv = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    cb1, cb2 = np.float32(1), np.float32(1)
    for t in range(1, 26):
        g = synth.normal(100 + t, n, 1e-2 * t)
        if t == 7:
            g[:3] = [np.nan, np.inf, -np.inf]
        cb1, cb2 = np.float32(cb1 * np.float32(0.9)), np.float32(cb2 * np.float32(0.999))
        oracle.lib.orc_adam(n, p, g, m, v, h["lr"], h["wd"], h["b1"], h["b2"], float(cb1), float(cb2), h["eps"])
        mp, mm, mv = torch_ref.adam(mp, g, mm, mv, float(cb1), float(cb2), **h)
        for what, a, b in (("param", p, mp), ("mean", m, mm), ("var", v, mv)):
            assert rel_l2(a, b) <= 1e-6, "t=%d %s: %.3e" % (t, what, rel_l2(a, b))
        # the next step starts from ONE state (the oracle's float32 one), as the teacher-forced GPU checks do
        mp, mm, mv = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    assert abs(float(cb1) - 0.9 ** 25) <= 1e-5 * 0.9 ** 25 and abs(float(cb2) - 0.999 ** 25) <= 1e-5


def test_committed_model_curves_reproduce():
    """the fixture's first two steps (the second one after an Adam update) recomputed by the generator's own code, every model"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import trajectory_curves as tc
    g = np.load(GOLDEN)
    assert int(g["steps"]) == 25 and int(g["batch"]) == 8
    bad = []
    for kind in tc.KINDS:  # (curve() fixes torch's thread count: the float32 sums depend on it)
        got = tc.curve(kind, int(g["batch"]), 2)
        bad += [(kind, s, float(got[s]), float(g[kind][s])) for s in range(2) if abs(got[s] - g[kind][s]) > 1e-6 * abs(g[kind][s])]
    assert not bad, bad
