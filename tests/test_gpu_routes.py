"""Every RESNET_MI_* switch (README, "Environment switches"; the table is tests/routes.py) per element and through whole training steps.

The switches are read once per process, so every (switch, value) runs in a child process of its own (tests/route_worker.py):

* test_route_table_names_every_switch (no GPU): the switches the code reads, the table and the README agree.
* test_operators_under_switch: the entry's operator cases through the perelement.py checkers (float64 reference, their bounds) with the
  switch set; the launch ring must show every variant name the entry expects and at least one name the default-route child did not
  launch on the same cases (a forced value the planner ignores proves nothing); "bitwise" entries are compared bit for bit with the
  default child's outputs.  One default child per base route (none, and RESNET_MI_IGEMM=0 for the direct kernels' knobs) is shared.
* test_trainer_under_switch: the whole-step checks re-run in a child with the switch set (fp32: test_training_step_parity on C1S and
  test_store_policies_bit_identical_after_25_steps[f32]; the bf16 switches are parameters of
  test_gpu_bf16.py::test_training_step_bf16_on_the_other_kernel_routes); "bitwise" entries also compare loss, every gradient and every
  parameter of two steps with a default child's, bit for bit.
* test_planner_names_the_launched_kernel: per RESNET_MI_IGEMM value (and once with RESNET_MI_BF16_PW_WGRAD=0) one child runs the fp32
  and bf16 operators over shapes that take every kernel of the two NCHW route families; the convolution launch in the ring carries the
  name of the kernel mi_layer_kernels answered, with exactly the re-layout and reduce launches that kernel implies.

A child that ends by a signal, times out or reports a GPU memory fault is a casualty: every later test of this file then fails at once
without starting another process on the device.  Nothing is retried.
"""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import routes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "route_worker.py")
CASUALTY = []   # the first child that died, timed out or faulted the device
WORST = {}      # (switch=value, variant names, checker key) -> worst distance, printed at the end of the module
TIMES = {}      # child -> wall seconds

OP_ENTRIES = [e for e in routes.ROUTES if e["cases"]]
F32_TRAINER = [e for e in routes.ROUTES if e["trainer"] in ("f32", "both")]
BITWISE_TRAINER = [e for e in routes.ROUTES if e["trainer"] and e["relation"] == "bitwise"]


def run_child(what, argv, env_add, timeout):
    """one child process under its own time limit; returns the CompletedProcess, or fails the test (and marks the casualty)"""
    if CASUALTY:
        pytest.fail("not started: an earlier child of this module was a casualty (%s)" % CASUALTY[0])
    env = dict(os.environ, **env_add)
    env.setdefault("RESNET_MI_TRACE", "1")
    t0 = time.time()
    try:
        r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    except subprocess.TimeoutExpired:
        CASUALTY.append("%s: no end after %d s" % (what, timeout))
        pytest.fail(CASUALTY[0])
    TIMES[what] = time.time() - t0
    text = r.stdout + r.stderr
    if r.returncode < 0 or r.returncode in (134, 137, 139) or "illegal memory access" in text or "Memory access fault" in text:
        CASUALTY.append("%s: exit status %d\n%s" % (what, r.returncode, text[-3000:]))
        pytest.fail(CASUALTY[0])
    return r


def ops_child(tmp, tag, keys, env_add):
    out = str(tmp / (tag + ".json"))
    r = run_child("operators " + tag, [sys.executable, WORKER, "ops", out] + keys, env_add, 600)
    assert r.returncode == 0, "%s\n%s" % (tag, (r.stdout[-3000:] + r.stderr[-3000:]))
    with open(out) as f:
        return json.load(f), np.load(out + ".npz")


def trainer_child(tmp, tag, which, env_add):
    out = str(tmp / (tag + ".json"))
    r = run_child("two steps " + tag, [sys.executable, WORKER, "trainer", out, which], env_add, 300)
    assert r.returncode == 0, "%s\n%s" % (tag, (r.stdout[-3000:] + r.stderr[-3000:]))
    return np.load(out + ".npz")


def _base_tag(base):
    return "default" + "".join("+%s=%s" % kv for kv in sorted(base.items()))


@pytest.fixture(scope="module")
def default_ops(tmp_path_factory):
    """per base route: the default child's results over the cases of every entry on that base (started on first use)"""
    tmp, done = tmp_path_factory.mktemp("routes_default"), {}

    def get(base):
        tag = _base_tag(base)
        if tag not in done:
            done[tag] = None    # a failure here is not repeated for the next entry
            done[tag] = ops_child(tmp, tag, [e["key"] for e in OP_ENTRIES if e["base"] == base], base)
        if done[tag] is None:
            pytest.fail("the default child %s failed (see the first test that needed it)" % tag)
        return done[tag]
    return get


@pytest.fixture(scope="module")
def default_trainer(tmp_path_factory):
    tmp, done = tmp_path_factory.mktemp("routes_trainer_default"), {}

    def get():
        if "d" not in done:
            done["d"] = None
            done["d"] = trainer_child(tmp, "default", "both", {})
        if done["d"] is None:
            pytest.fail("the default trainer child failed (see the first test that needed it)")
        return done["d"]
    return get


@pytest.fixture(scope="module", autouse=True)
def _summary():
    t0 = time.time()
    yield
    print("\nworst distance per switch, variant and op (fp32 and reductions: x 2^-24 A or sum|terms|, bf16: bf16 ulps); module %.0f s" % (time.time() - t0))
    for key in sorted(WORST):
        print("  %-28s %-9s %s  %s  %.3g" % (key[0], routes.by_key(key[0])["relation"], key[1], key[2], WORST[key]))
    print("children, wall seconds: " + ", ".join("%s %.0f" % kv for kv in sorted(TIMES.items())))


# ---------------------------------------------------------------------------------------------------------------------------
def _quoted_switches(text):
    return set(re.findall(r"\"(RESNET_MI_[A-Z0-9_]+)\"", text))


def test_route_table_names_every_switch():
    """the switches the library reads (quoted RESNET_MI_* strings of resnet_amd/csrc/* and binding.py) are all in ROUTES or EXEMPT, the
    table names none the code does not read, and the README's "Environment switches" paragraph names only switches the code reads -- and
    every one of them"""
    read = set()
    csrc = os.path.join(ROOT, "resnet_amd", "csrc")
    for fn in sorted(os.listdir(csrc)) + [os.path.join("..", "binding.py")]:
        path = os.path.join(csrc, fn)
        if os.path.isfile(path) and not fn.endswith((".o", ".so")):
            with open(path, errors="replace") as f:
                read |= _quoted_switches(f.read())
    assert len(read) >= 25, sorted(read)
    table = {e["switch"] for e in routes.ROUTES}
    assert not table & set(routes.EXEMPT), "in both ROUTES and EXEMPT: %s" % sorted(table & set(routes.EXEMPT))
    assert read - table - set(routes.EXEMPT) == set(), "read by the code, in neither ROUTES nor EXEMPT: %s" % sorted(read - table - set(routes.EXEMPT))
    assert (table | set(routes.EXEMPT)) - read == set(), "in the table, read by no code: %s" % sorted((table | set(routes.EXEMPT)) - read)
    keys = [e["key"] for e in routes.ROUTES]
    assert len(keys) == len(set(keys))
    for e in routes.ROUTES:
        assert e["relation"] in ("bitwise", "bounds") and e["why"]
        assert e["cases"] or e["trainer"], e["key"]
        assert bool(e["cases"]) == bool(e["names"]), "%s: operator cases and expected variant names go together" % e["key"]
    assert all(routes.EXEMPT.values())
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    start = readme.index("Environment switches")
    para = readme[start:readme.index("\n\n", start)]
    named = set(re.findall(r"RESNET_MI_[A-Z0-9_]+", para))
    assert named - read == set(), "the README names switches no code reads: %s" % sorted(named - read)
    assert read - named == set(), "the README's paragraph leaves out: %s" % sorted(read - named)
    assert "RESNET_MI_IGEMM=0|1|2`" in para, "RESNET_MI_IGEMM takes 0, 1 or 2"


@pytest.mark.gpu
@pytest.mark.parametrize("net", ["c4i", "c1s"])
def test_trainer_table_is_the_planners_answer(net):
    """a live trainer's table (mi_debug_trainer_routes) holds, convolution by convolution, what mi_layer_routes answers for the stem and for
    convref.trainer_units(dims) with the trainer's storage type, store policy and batch: fp32 under every policy, bf16 under FAST and
    RECOMPUTE_BN (batch 4, 32 x 32 input)"""
    import convref as R
    from resnet_amd import Trainer
    from resnet_amd import binding as B
    dims, N = R.nets()[net], 4
    tr = Trainer(dims, N)
    try:
        assert tr.L.mi_device_count() >= 1, "no HIP device"
        shapes = [(R.stem_shape(dims), 0)] + [(u[2], u[3]) for u in R.trainer_units(dims)]
        for dtype, policies in ((B.MI_DTYPE_F32, (B.MI_STORE_FAST, B.MI_STORE_RECOMPUTE_BN, B.MI_STORE_FULL)),
                                (B.MI_DTYPE_BF16, (B.MI_STORE_FAST, B.MI_STORE_RECOMPUTE_BN))):
            tr.set_store_policy(B.MI_STORE_FAST)
            tr.set_dtype(dtype)
            for policy in policies:
                tr.set_store_policy(policy)
                want = [R.layer_routes(tr.L, dtype, policy, N, *shape, site=site) for shape, site in shapes]
                assert None not in want
                assert tr.routes() == want, (net, dtype, policy)
    finally:
        tr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key", [e["key"] for e in OP_ENTRIES])
def test_operators_under_switch(key, default_ops, tmp_path):
    e = routes.by_key(key)
    base, base_raw = default_ops(e["base"])
    got, got_raw = ops_child(tmp_path, key.replace("=", "_"), [key], routes.env_of(e))
    ids = [routes.case_id(c) for c in e["cases"]]
    assert got["checked"] == len(ids) == len(set(ids)) and sorted(got["cases"]) == sorted(ids), "cases checked %d, listed %d" % (got["checked"], len(ids))
    launched = {n for cid in ids for n in got["cases"][cid]["names"]}
    default_launched = {n for cid in ids for n in base["cases"][cid]["names"]}
    print("%s launched %s\ndefault launched %s" % (key, sorted(launched), sorted(default_launched)))
    new = sorted(launched - default_launched)
    for cid in ids:
        for k, w in got["cases"][cid]["worst"].items():
            # the names of this case that the default run of the same case lacks: the variant this distance belongs to
            variant = ", ".join(sorted(set(got["cases"][cid]["names"]) - set(base["cases"][cid]["names"]))) or "(the default's kernels)"
            WORST[(key, variant, k)] = max(WORST.get((key, variant, k), 0.0), w)
    missing = [n for n in e["names"] if n not in launched]
    assert not missing, "%s: expected variants not launched: %s\nlaunched: %s" % (key, missing, sorted(launched))
    assert new, "%s launched nothing the default route does not launch on the same cases: the switch was ignored\n%s" % (key, sorted(launched))
    if e["relation"] == "bitwise":
        for cid in ids:
            ka, kb = got["cases"][cid]["raw"], base["cases"][cid]["raw"]
            assert ka and len(ka) == len(kb), "%s: raw outputs saved %d, default %d" % (cid, len(ka), len(kb))
            for a, b in zip(ka, kb):
                x, y = got_raw[a], base_raw[b]
                assert x.dtype == y.dtype and x.shape == y.shape, cid
                assert x.tobytes() == y.tobytes(), "%s under %s: output %s differs from the default route's in %d of %d elements" \
                    % (cid, key, a, int(np.count_nonzero(x != y)), x.size)


@pytest.mark.gpu
@pytest.mark.parametrize("key", [e["key"] for e in F32_TRAINER] + [e["key"] for e in BITWISE_TRAINER if e["trainer"] == "bf16"])
def test_trainer_under_switch(key, default_trainer, tmp_path):
    e = routes.by_key(key)
    env = routes.env_of(e)
    if e["trainer"] in ("f32", "both"):
        r = run_child("whole-step checks " + key,
                      [sys.executable, "-m", "pytest", os.path.join(HERE, "test_gpu_net.py") + "::test_training_step_parity[C1S]",
                       os.path.join(HERE, "test_gpu_trajectory.py") + "::test_store_policies_bit_identical_after_25_steps[f32]",
                       "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"], env, 900)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        assert "2 passed" in r.stdout, r.stdout[-2000:]
    if e["relation"] == "bitwise":
        ref = default_trainer()
        got = trainer_child(tmp_path, key.replace("=", "_"), e["trainer"], env)
        assert len(got.files) > 10
        for name in got.files:
            assert got[name].tobytes() == ref[name].tobytes(), "%s under %s differs from the default trainer's" % (name, key)


# ---------------------------------------------------------------------------------------------------------------------------
# (dtype, op, C, H, K, k, stride, N, addend) of test_planner_names_the_launched_kernel
def _kernel_cases():
    from test_gpu_ops import DIRECT
    f32 = [(64, 8, 96, 3, 1, 2),                                  # the mixed layer: another kernel per operation
           routes.S_3x3, routes.S_1x1, routes.S_3x3s2, routes.S_49,
           (48, 8, 96, 1, 1, 4),                                  # a 1x1 no implicit GEMM tiles: gemm_mfma_kernel in every mode
           (256, 56, 64, 1, 1, 8),                                # the weight gradient's grouped split reduce
           (3, 32, 64, 7, 2, 4)]                                  # the stem
    bf16 = [(256, 8, 128, 1, 1, 5), (128, 14, 256, 1, 1, 3),      # pw_wgrad_kernel unless switched off
            (192, 8, 128, 1, 1, 5)]                               # C % 128 != 0: bgemm_kernel
    cases = [("f32", c[0]) + tuple(c[1:7]) + (c[7],) for c in DIRECT]
    cases += [("f32", op) + sh + (False,) for sh in f32 for op in routes.ALL if not (sh[3] == 7 and op == "dgrad")]
    cases += [("bf16", op) + sh + (False,) for sh in bf16 for op in routes.ALL]
    return list(dict.fromkeys(cases))


# what the issue of this test states outright, (dtype, op, shape) -> kernel name per RESNET_MI_IGEMM value (None: every value)
KERNEL_FACTS = [
    (("f32", "fwd", (64, 8, 96, 3, 1, 2)), {"2": "dconv_kernel", "0": "dconv_kernel"}),       # K % 64 != 0
    (("f32", "dgrad", (64, 8, 96, 3, 1, 2)), {"2": "igemm_kernel", "0": "dconv_kernel"}),
    (("f32", "wgrad", (64, 8, 96, 3, 1, 2)), {"2": "wgradC_kernel", "0": "wgradC_kernel"}),
    (("f32", "fwd", (48, 8, 96, 1, 1, 4)), {None: "gemm_mfma_kernel"}),
    (("f32", "dgrad", (48, 8, 96, 1, 1, 4)), {None: "gemm_mfma_kernel"}),
    (("f32", "wgrad", (48, 8, 96, 1, 1, 4)), {None: "gemm_mfma_kernel"}),
    (("f32", "fwd", routes.S_3x3), {"0": "dconv_kernel", "1": "dconv_kernel", "2": "igemm_kernel"}),
    (("f32", "fwd", routes.S_1x1), {"0": "gemm_mfma_kernel", "1": "gemm_mfma_kernel", "2": "igemm_kernel"}),
    (("f32", "wgrad", routes.S_1x1), {"0": "gemm_mfma_kernel", "1": "igemm_kernel", "2": "igemm_kernel"}),
    (("f32", "fwd", (3, 32, 64, 7, 2, 4)), {"0": "dconv_kernel", "2": "st32_fwd_kernel"}),
    (("f32", "wgrad", (3, 32, 64, 7, 2, 4)), {"0": "wgrad_kernel", "2": "st32_wgrad_kernel"}),
    (("bf16", "wgrad", (192, 8, 128, 1, 1, 5)), {None: "bgemm_kernel"}),
    (("bf16", "fwd", (256, 8, 128, 1, 1, 5)), {None: "bgemm_kernel"}),
]


@pytest.mark.gpu
@pytest.mark.parametrize("env_add", [{"RESNET_MI_IGEMM": "0"}, {"RESNET_MI_IGEMM": "1"}, {"RESNET_MI_IGEMM": "2"}, {"RESNET_MI_BF16_PW_WGRAD": "0"}],
                         ids=["igemm0", "igemm1", "igemm2", "pw_wgrad0"])
def test_planner_names_the_launched_kernel(env_add, tmp_path):
    """Per case and operation the child clears the launch ring and runs the operator; here: the one convolution kernel among the ring's
    names is the kernel mi_layer_kernels named (binding.MI_KERNEL_NAMES), for the cases KERNEL_FACTS lists it is also the kernel the
    shape rules give, and the launches around it are the ones that kernel implies -- an operator has no pre-laid weights, so
    igemm_wt_kernel exactly in front of an implicit-GEMM forward or 3x3 dgrad and wt_relayout_kernel exactly in front of dconv_kernel;
    split_reduce_kernel only behind the kernels that split (wgradC_kernel, wgrad_kernel, gemm_mfma_kernel), the implicit GEMM's own
    reduce exactly behind its weight gradient, grouped where mi_conv_plan says so.  The RESNET_MI_BF16_PW_WGRAD=0 child runs the bf16
    cases only."""
    from resnet_amd import binding as B
    cases = [c for c in _kernel_cases() if "RESNET_MI_IGEMM" in env_add or c[0] == "bf16"]
    with open(tmp_path / "cases.json", "w") as f:
        json.dump(cases, f)
    out = str(tmp_path / "kernels.json")
    r = run_child("kernels %s" % env_add, [sys.executable, WORKER, "kernels", out, str(tmp_path / "cases.json")], env_add, 300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        got = json.load(f)["cases"]
    assert len(got) == len(cases)
    conv_names = set(B.MI_KERNEL_NAMES[1:])
    mode, pw = env_add.get("RESNET_MI_IGEMM"), env_add.get("RESNET_MI_BF16_PW_WGRAD")
    seen = set()
    for g in got:
        dt, op, Cn, H, K, k, s, N, addend = g["case"]
        what = "%s under %s" % (g["case"], env_add)
        want = B.MI_KERNEL_NAMES[g["kernel"]]
        heads = [n.split("<")[0] for n in g["names"]]
        print("%-60s %-18s %s" % (g["case"], want, g["names"]))
        # (the stem's weight-gradient operator runs the forward first: the weight gradient reads the planes it leaves)
        behind = {"st32_wgrad_kernel": {"st32_fwd_kernel"}, "st_wgrad_kernel": {"st_fwd_kernel"}}.get(want, set())
        assert want and {h for h in heads if h in conv_names} - behind == {want}, "%s: the planner names %r, launched %s" % (what, want, g["names"])
        seen.add(want)
        for (fdt, fop, fshape), by_mode in KERNEL_FACTS:
            if (fdt, fop, tuple(fshape)) == (dt, op, (Cn, H, K, k, s, N)) and (None in by_mode or mode in by_mode):
                assert want == by_mode.get(None, by_mode.get(mode)), what
        if dt == "bf16" and op == "wgrad" and Cn % 128 == 0:
            assert want == ("bgemm_kernel" if pw == "0" else "pw_wgrad_kernel"), what
        assert ("igemm_wt_kernel" in heads) == (want == "igemm_kernel" and (op == "fwd" or (op == "dgrad" and k == 3))), what
        assert ("wt_relayout_kernel" in heads) == (want == "dconv_kernel"), what
        if "split_reduce_kernel" in heads:
            assert want in ("wgradC_kernel", "wgrad_kernel", "gemm_mfma_kernel") and op == "wgrad", what
        ig_reduce = [n for n in g["names"] if n.startswith("igemm_wgrad_reduce")]
        if dt == "f32":
            assert (g["plan"] is not None) == (want == "igemm_kernel"), "%s: mi_conv_plan and mi_layer_kernels disagree" % what
            assert len(ig_reduce) == (1 if want == "igemm_kernel" and op == "wgrad" else 0), what
            if ig_reduce and not ig_reduce[0].startswith("igemm_wgrad_reduce_t_kernel"):
                assert ("grouped" in ig_reduce[0]) == bool(g["plan"][6]), what
    if mode == "2":
        assert {"igemm_kernel", "gemm_mfma_kernel", "dconv_kernel", "wgradC_kernel", "wgrad_kernel", "bgemm_kernel", "pw_wgrad_kernel",
                "st32_fwd_kernel", "st32_wgrad_kernel"} <= seen, sorted(seen)
        assert any("grouped" in n for g in got for n in g["names"]), "no case reached the grouped split reduce"
