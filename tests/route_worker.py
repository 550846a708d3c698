"""Child process of test_gpu_routes.py: the switches under test are in this process's environment (the library reads each once).

  route_worker.py ops OUT.json KEY [KEY ...]       the operator cases of the table entries KEY (tests/routes.py), each case once
  route_worker.py trainer OUT.json f32|bf16|both   two training steps at batch 4: C1S in fp32, C4I in bf16
  route_worker.py kernels OUT.json CASES.json      per case (dtype, op, C, H, K, k, stride, N, addend): what the planner names, what was launched

ops: per case, clear the launch ring, run the case's perelement.py checker (float64 reference, the checker's own bounds: a failure ends
the process with a traceback), and record the worst distances and the ring's names.  For the cases of "bitwise" entries the operator is
run once more on the same operands and its raw outputs go to OUT.json.npz.  trainer: loss, every gradient of both steps and every
parameter after them go to OUT.json.npz.  kernels: per case, the planner's routes and kernel ids (mi_layer_routes, mi_layer_kernels), the
fp32 weight gradient's plan (mi_conv_plan), then the launch ring cleared, the operator of the planned route run once and the ring's names
(nothing is compared here: the parent asserts).  OUT.json is written last: it exists only if everything before it passed.
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import convref as R  # noqa: E402
import perelement as P  # noqa: E402
import routes  # noqa: E402
import synth  # noqa: E402


def ring_names(L):
    buf = ctypes.create_string_buffer(96 * 100)
    n = L.mi_debug_trace_names(buf, len(buf))
    names = buf.value.decode().split("\n")[:-1]
    assert n == len(names), "the ring holds %d names, %d were returned" % (n, len(names))
    return names


def check(ops, kind, case, N, record):
    if kind == "conv":
        P.conv_route(ops, case, N, record)
    elif kind == "conv_bn":
        P.conv_bn_fwd(ops, case[0], N, record, route=case[1])
    elif kind == "dgrad_bn":
        P.dgrad_bn_bwd(ops, case, N, record)
    elif kind == "bn_fwd":
        P.bn_fwd(ops, case, N, record)
    elif kind == "bn_bwd":
        P.bn_bwd(ops, case, N, record)
    elif kind == "stem":
        P.stem(ops, case[0], case[1], N, case[2], record)
    else:
        raise ValueError(kind)


def raw(ops, kind, case, N):
    """the operator's own outputs on the checker's operands, as a flat list of arrays"""
    if kind == "conv":
        out = [P.conv_route_call(ops, case, P.conv_route_inputs(case, N))]
    elif kind == "conv_bn":
        out = P.conv_bn_fwd_call(ops, case[0], P.conv_bn_fwd_inputs(case[0], N), case[1])
    elif kind == "dgrad_bn":
        out = P.dgrad_bn_bwd_call(ops, case, P.dgrad_bn_bwd_inputs(case, N))
    elif kind == "bn_fwd":
        inp = P.bn_fwd_inputs(case, N)
        out = [a for form in case[3] for a in P.bn_fwd_call(ops, case, inp, form)]
    elif kind == "bn_bwd":
        out = P.bn_bwd_call(ops, case, P.bn_bwd_inputs(case, N))
    else:
        out = [P.stem_call(ops, case[0], case[1], P.stem_inputs(case[0], case[1], N, case[2]))]
    return [np.ascontiguousarray(a) for a in out if isinstance(a, np.ndarray)]


def run_ops(out_path, keys):
    from resnet_amd.ops import Ops
    ops = Ops()
    assert ops.L.mi_device_count() >= 1, "no HIP device"
    R.set_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))
    entries = [routes.by_key(k) for k in keys]
    bitwise = {routes.case_id(c) for e in entries if e["relation"] == "bitwise" for c in e["cases"]}
    result, arrays = {}, {}
    for i, (kind, case, N) in enumerate(routes.union_cases(entries)):
        cid = routes.case_id((kind, case, N))
        worst = {}

        def record(key, w):
            k = " / ".join(str(x) for x in key)
            worst[k] = max(worst.get(k, 0.0), float(w))
        ops.L.mi_debug_trace_clear()
        check(ops, kind, case, N, record)
        names = ring_names(ops.L)
        assert names, "%s launched nothing the ring saw (RESNET_MI_TRACE must be on)" % cid
        result[cid] = dict(worst=worst, names=names, raw=[])
        if cid in bitwise:
            for j, a in enumerate(raw(ops, kind, case, N)):
                arrays["c%d_%d" % (i, j)] = a
                result[cid]["raw"].append("c%d_%d" % (i, j))
    np.savez(out_path + ".npz", **arrays)
    with open(out_path, "w") as f:
        json.dump(dict(cases=result, checked=len(result)), f)


def run_kernels(out_path, cases_path):
    from resnet_amd import binding as B
    from resnet_amd.ops import Ops, layer_kernels, layer_routes
    ops = Ops()
    assert ops.L.mi_device_count() >= 1, "no HIP device"
    with open(cases_path) as f:
        cases = [tuple(c) for c in json.load(f)]
    result = []
    for dt, op, Cn, H, K, k, s, N, addend in cases:
        i = ("fwd", "dgrad", "wgrad").index(op)
        dtype = B.MI_DTYPE_BF16 if dt == "bf16" else B.MI_DTYPE_F32
        route, kernel = layer_routes(ops.L, dtype, B.MI_STORE_FAST, N, Cn, H, K, k, s), layer_kernels(ops.L, dtype, B.MI_STORE_FAST, N, Cn, H, K, k, s)
        assert route is not None and kernel is not None, "the planner refuses %s" % ((dt, op, Cn, H, K, k, s, N),)
        plan = R.conv_plan(ops.L, 0, "default", op, N, Cn, H, K, k, s) if dt == "f32" else None
        ops.L.mi_debug_trace_clear()
        if route[i] in ((B.MI_FWD_STEM_F32, B.MI_FWD_STEM_BF16) if op == "fwd" else (B.MI_WG_STEM_F32, B.MI_WG_STEM_BF16)) and k == 7:
            got = P.stem_call(ops, dt, op, P.stem_inputs(dt, op, N, H))
        else:
            assert route[i] == (1 if dt == "bf16" else 0), "the planned route of %s is %d: not an operator this worker runs" % ((dt, op, Cn, H, K, k, s, N), route[i])
            case = (dt, "default", op, Cn, H, K, k, s, "red" if addend else "")
            got = P.conv_route_call(ops, case, P.conv_route_inputs(case, N))
        assert got is not None
        result.append(dict(case=[dt, op, Cn, H, K, k, s, N, addend], route=route[i], kernel=kernel[i], plan=plan, names=ring_names(ops.L)))
    with open(out_path, "w") as f:
        json.dump(dict(cases=result), f)


HYPER = dict(lr=1e-4, wd=0.0, b1=0.9, b2=0.999, eps=1e-7)


def run_trainer(out_path, which):
    from resnet_amd import Trainer
    from resnet_amd import binding as B
    arrays = {}
    for tag, dims, dtype in (("f32", synth.C1S_DIMS, B.MI_DTYPE_F32), ("bf16", synth.C4I_DIMS, B.MI_DTYPE_BF16)):
        if which not in (tag, "both"):
            continue
        batch = 4
        tr = Trainer(dims, batch, **HYPER)
        assert tr.L.mi_device_count() >= 1, "no HIP device"
        tr.set_dtype(dtype)
        tr.set_params(synth.make_params(dims, perturb_bn=True))
        tr.source_host(B.MI_LAYOUT_NHWC)
        for step in range(2):
            im, lab = synth.make_batch(dims, batch, step=step)
            tr.fill_host_batch(im, lab)
            tr.load_new_batch()
            tr.forward()
            arrays["%s_loss%d" % (tag, step)] = np.float64(tr.loss()[0])
            tr.backward()
            tr.check()
            for i in range(tr.n_locations):
                arrays["%s_grad%d_%03d" % (tag, step, i)] = tr.get("grads", i)
            tr.update()
            tr.check()
        for i in range(tr.n_locations):
            arrays["%s_param_%03d" % (tag, i)] = tr.get("params", i)
        assert all(np.all(np.isfinite(a)) for a in arrays.values())
        tr.close()
    np.savez(out_path + ".npz", **arrays)
    with open(out_path, "w") as f:
        json.dump(dict(saved=sorted(arrays)), f)


if __name__ == "__main__":
    mode, out = sys.argv[1], sys.argv[2]
    if mode == "ops":
        run_ops(out, sys.argv[3:])
    elif mode == "kernels":
        run_kernels(out, sys.argv[3])
    else:
        run_trainer(out, sys.argv[3])
