"""Evaluation on the device (include/resnet_mi.h, "evaluation"): the running-statistics kernel, the eval pass, its metrics, the
checkpoint.  The model is tests/evalref.py, pinned against torch.nn.BatchNorm2d by tests/test_eval_model.py.

Every test calls a symbol the library did not have before.  Shapes are the smallest that cross each code path: the kernel on layers of
64, 3, 2048, 1 and 130 channels (below, at and across the 256-thread block and the 64-lane wave; several layers inside one block and
one layer across nine), the eval pass on every trainer configuration whose forward routes differ (fp32 / bf16, matrix-core and VALU
stem, odd tiles, the channel-last and LDS-DMA routes of ResNet-50, the BN-written channel-last planes, both store policies).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import evalref as E
import lossref as R
import synth
import torch_ref as T
from util import ACT_REL_L2, rel_l2

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
IN48_DIMS = synth.resnet_dims(input=48, n_conv_blocks=1, reductions=(), final_depth=256)
NETS = {"C1": (synth.C1_DIMS, 4), "C1S": (synth.C1S_DIMS, 4), "C1S_batch5": (synth.C1S_DIMS, 5), "C4I": (synth.C4I_DIMS, 4),
        "C1_in48": (IN48_DIMS, 3), "R50": (synth.R50_DIMS, 2)}
_PARAMS = {}


def _params(dims):
    key = (dims["input"], dims["n_conv_blocks"], tuple(dims["is_block_spatial_reduction"]))
    if key not in _PARAMS:
        _PARAMS[key] = synth.make_params(dims, perturb_bn=True)
    return _PARAMS[key]


def _trainer(dims, batch, dtype=F32, policy=None, momentum=0.1, track=True, **kw):
    from resnet_amd import Trainer
    from resnet_amd import binding as B
    tr = Trainer(dims, batch, **kw)
    if tr.L.mi_device_count() < 1:
        pytest.fail("no HIP device: this test must run on the MI355X box")
    if policy is not None:
        tr.set_store_policy(policy)
    tr.set_dtype(dtype)
    tr.set_params(_params(dims))
    tr.source_host(B.MI_LAYOUT_NHWC)
    if track:
        tr.track_running_stats(momentum)
    return tr


def _load(tr, dims, batch, step):
    im, lab = synth.make_batch(dims, batch, step=step)
    tr.fill_host_batch(im, lab)
    tr.load_new_batch()
    return im, lab


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _batch_stats(tr, dims):
    names = E.bn_names(dims)
    return (np.concatenate([tr.activation(n + "means") for n in names]), np.concatenate([tr.activation(n + "vars") for n in names]))


# ---- 1. the kernel on its own ----
KERNEL_C = [64, 3, 2048, 1, 130]
KERNEL_N = [2, 1, 2, 2, 1]   # samples per channel: n = 1 is the unbias = 1 case
SLACK, GUARD = 5, 16         # arena words past the layers' sum (they belong to no layer); guard words around the arena
_KERNEL = {}


def _kernel_run(ops):
    """two successive updates, momentum 0.1 then 1 -- computed once, never written"""
    if not _KERNEL:
        rng = np.random.RandomState(21)
        stats = [[(rng.randn(c).astype(np.float32) * 3, (rng.rand(c).astype(np.float32) + 0.05) * 4) for c in KERNEL_C] for _ in range(2)]
        total = sum(KERNEL_C)
        start = np.stack([rng.randn(total + SLACK), rng.rand(total + SLACK) + 0.5]).astype(np.float32)
        fill = np.float32(-12345.5)
        first = ops.bn_running_update([m for m, _ in stats[0]], [v for _, v in stats[0]], KERNEL_N, start, 0.1, guard=GUARD, fill=fill)
        second = ops.bn_running_update([m for m, _ in stats[1]], [v for _, v in stats[1]], KERNEL_N, first[0], 1.0, guard=GUARD, fill=fill)
        _KERNEL.update(stats=stats, start=start, first=first, second=second, fill=fill, total=total)
    return _KERNEL


@pytest.mark.parametrize("which", ["momentum_0.1", "momentum_1"])
def test_running_update_kernel(ops, which):
    k = _kernel_run(ops)
    step = 0 if which == "momentum_0.1" else 1
    m = (0.1, 1.0)[step]
    old = (k["start"], k["first"][0])[step].astype(np.float64)
    new, front, back = (k["first"], k["second"])[step]
    total = k["total"]
    mean = np.concatenate([a for a, _ in k["stats"][step]]).astype(np.float64)
    var = np.concatenate([a for _, a in k["stats"][step]]).astype(np.float64)
    ub = np.concatenate([np.full(c, np.float64(E.unbias(n))) for c, n in zip(KERNEL_C, KERNEL_N)])
    assert ub[64] == 1.0 and ub[0] == 2.0  # (the 3-channel layer has n = 1)
    mf = np.float64(np.float32(m))
    want_m = (1 - mf) * old[0, :total] + mf * mean
    want_v = (1 - mf) * old[1, :total] + mf * (var * ub)
    # the roundings of 1 - m and (1 - m) old are relative to |old|, those of var unbias and m (...) to |stat| unbias, that of the sum to
    # the result: at most 2^-24 (3 |old| + 3 |stat| unbias), inside the stated 4 2^-24 (|old| + |stat| unbias)
    bound_m = 4 * 2.0 ** -24 * (np.abs(old[0, :total]) + np.abs(mean))
    bound_v = 4 * 2.0 ** -24 * (np.abs(old[1, :total]) + np.abs(var) * ub)
    err_m, err_v = np.abs(new[0, :total] - want_m), np.abs(new[1, :total] - want_v)
    print("%s: worst |error| / bound: means %.3f, vars %.3f" % (which, float(np.max(err_m / bound_m)), float(np.max(err_v / bound_v))))
    assert np.all(err_m <= bound_m) and np.all(err_v <= bound_v)
    if m == 1.0:
        assert _same(new[0, :total], np.concatenate([a for a, _ in k["stats"][step]])), "momentum 1: the means are the batch means"
    # words of no layer, and the guard words around the arena
    assert _same(new[:, total:], (k["start"], k["first"][0])[step][:, total:])
    assert np.all(front == k["fill"]) and np.all(back == k["fill"]) and front.size == back.size == GUARD


# ---- 2. eval equals the training forward when the statistics are the batch's ----
FWD_NAMES = ["init_conv_applied", "init_conv_activated", "init_convblock_input", "max_inds", "final_avg_pool", "fc_output", "softmax"]
BLOCK_NAMES = ["reduction_applied", "reduction_activated", "spatial_applied", "spatial_activated", "expanded_applied", "transformed_residual",
               "post_projection_norm_vals", "output_activated"]
SHARED_UNDER_RECOMPUTE = {"init_conv_activated", "reduction_activated", "spatial_activated", "post_projection_norm_vals"}
SAME_CASES = [("C1", F32, "FAST"), ("C1S_batch5", F32, "FAST"), ("C1_in48", F32, "FAST"), ("C1S_batch5", F32, "RECOMPUTE_BN"),
              ("C1", BF16, "FAST"), ("C1S", BF16, "FAST"), ("C1S_batch5", BF16, "FAST"), ("C4I", BF16, "FAST"), ("C1_in48", BF16, "FAST"),
              ("C1S_batch5", BF16, "RECOMPUTE_BN"), ("R50", F32, "FAST"), ("R50", BF16, "FAST"), ("R50", BF16, "RECOMPUTE_BN")]


def _stored(tr, dims, recompute):
    names = list(FWD_NAMES)
    for b in range(dims["n_conv_blocks"]):
        k = tr.t.contents.forward_buffer.contents.activations.contents.activation_conv_blocks[b].contents
        for leaf in BLOCK_NAMES:
            if leaf in ("transformed_residual", "post_projection_norm_vals") and not k.transformed_residual:
                continue
            names.append("conv_blocks/%02d/%s" % (b, leaf))
    if recompute:  # the BN(+ReLU) tensors are two shared scratch buffers under this policy: each holds its last writer only
        names = [n for n in names if n.split("/")[-1] not in SHARED_UNDER_RECOMPUTE]
    return {n: tr.activation(n) for n in names}


@pytest.mark.parametrize("case", SAME_CASES, ids=["%s-%s-%s" % (n, ("f32", "bf16")[d], p) for n, d, p in SAME_CASES])
def test_eval_with_the_batch_statistics_is_the_training_forward(case):
    from resnet_amd import binding as B
    net, dtype, policy = case
    dims, batch = NETS[net]
    tr = _trainer(dims, batch, dtype, getattr(B, "MI_STORE_" + policy))
    try:
        _load(tr, dims, batch, 0)
        tr.forward()
        tr.check()
        means, vars_ = _batch_stats(tr, dims)
        assert means.size == sum(E.bn_channels(dims)) == tr.L.mi_trainer_running_stats_channels(tr.t)
        train = _stored(tr, dims, policy == "RECOMPUTE_BN")
        assert tr.running_updates() == 1
        tr.set_running_stats(means, vars_)
        tr.eval_forward()
        tr.check()
        got = _stored(tr, dims, policy == "RECOMPUTE_BN")
        for name in train:
            diff = int(np.sum(_bits(train[name]) != _bits(got[name])))
            assert diff == 0, "%s: %d of %d elements differ from the training forward" % (name, diff, train[name].size)
        # the pass wrote neither the caches, nor the running statistics, nor the counter
        m2, v2 = _batch_stats(tr, dims)
        assert _same(m2, means) and _same(v2, vars_)
        rm, rv = tr.running_stats()
        assert _same(rm, means) and _same(rv, vars_) and tr.running_updates() == 1
    finally:
        tr.close()


# ---- 3. semantics against the independent model ----
def test_running_statistics_and_eval_logits_against_the_model(ops):
    dims, batch, m = synth.C1S_DIMS, 4, 0.1
    tr = _trainer(dims, batch, momentum=m)
    ref64, ref32 = E.EvalNet(dims, _params(dims), momentum=m), E.EvalNet(dims, _params(dims), momentum=m, dtype=torch.float32)
    try:
        assert tr.running_updates() == 0
        rm, rv = tr.running_stats()
        assert np.all(rm == 0) and np.all(rv == 1)
        for step in range(3):
            im, lab = _load(tr, dims, batch, step)
            tr.forward()
            for ref in (ref64, ref32):
                ref.forward(T.nhwc_to_nchw(im), lab)
        tr.check()
        assert tr.running_updates() == 3 and [s["updates"] for s in ref64.state] == [3] * len(ref64.state)
        rm, rv = tr.running_stats()
        (m64, v64), (m32, v32) = ref64.running(), ref32.running()
        at = np.cumsum([0] + E.bn_channels(dims))
        for i, name in enumerate(E.bn_names(dims)):
            s = slice(at[i], at[i + 1])
            for what, got, r64, r32 in (("means", rm, m64, m32), ("vars", rv, v64, v32)):
                e_gpu, e_f32 = rel_l2(got[s], r64[s]), rel_l2(r32[s], r64[s])
                print("%s%s: HIP %.2e, fp32 model %.2e" % (name, what, e_gpu, e_f32))
                assert e_gpu <= 3 * e_f32 + ACT_REL_L2, "running %s of %s: HIP %.3e, fp32 model %.3e vs the float64 model" % (what, name, e_gpu, e_f32)
        im, lab = synth.make_batch(dims, batch, step=3)
        x = T.nhwc_to_nchw(im)
        tr.eval_forward(x, lab, topk=5)
        tr.check()
        logits = tr.activation("fc_output")
        l64, l32 = ref64.eval_forward(x), ref32.eval_forward(x).astype(np.float64)
        e_gpu, e_f32 = rel_l2(logits, l64), rel_l2(l32, l64)
        print("eval logits: HIP %.2e, fp32 model %.2e" % (e_gpu, e_f32))
        assert e_gpu <= 3 * e_f32 + ACT_REL_L2, (e_gpu, e_f32)
        assert tr.running_updates() == 3 and _same(tr.running_stats()[0], rm)
        # the metrics: lossref on the product's own logits -- counts exact, loss_sum inside the summed row bounds
        last, total = tr.eval_metrics()
        _, _, row_loss, rank = R.loss_head(logits, lab, 0.0)
        assert (last["rows"], last["batches"]) == (batch, 1) and total == last
        assert last["wrong_top1"] == int(np.sum(rank >= 1)) and last["wrong_topk"] == int(np.sum(rank >= 5))
        assert abs(last["loss_sum"] - row_loss.sum()) <= R.loss_bound(row_loss).sum(), (last["loss_sum"], row_loss.sum())
        assert _same(tr.activation("softmax"), ops.softmax(logits))
    finally:
        tr.close()


# ---- 4. padding rows do not exist ----
def test_rows_past_n_valid_change_nothing():
    from resnet_amd import binding as B
    dims, batch = synth.C1S_DIMS, 5
    tr = _trainer(dims, batch)
    try:
        assert tr.L.mi_trainer_set_loss(tr.t, 0.0, 5, B.MI_LOSS_DEVICE) == 0, tr.error()
        _load(tr, dims, batch, 0)
        tr.forward()  # (running statistics that are not the initial ones, and a training record)
        records = tr.metrics()
        x = T.nhwc_to_nchw(synth.make_batch(dims, batch, step=1)[0])
        other = T.nhwc_to_nchw(synth.make_batch(dims, batch, step=2)[0])
        lab = synth.make_batch(dims, batch, step=1)[1]
        tr.eval_forward(x[:3], lab[:3])  # rows 3 and 4 are zero images
        short = tr.activation("fc_output")
        last3 = tr.eval_metrics()[0]
        pred3 = tr.activation("softmax")
        tr.eval_forward(np.concatenate([x[:3], other[3:]]), lab)
        full = tr.activation("fc_output")
        last5 = tr.eval_metrics()[0]
        tr.check()
        assert _same(short[:3], full[:3]) and not _same(short[3:], full[3:])
        assert last3["rows"] == 3 and last5["rows"] == 5 and last3["batches"] == 1
        assert _same(pred3[:3], tr.activation("softmax")[:3])
        rank = R.rank_of(pred3[:3], lab[:3])
        assert last3["wrong_top1"] == int(np.sum(rank >= 1)) and last3["wrong_topk"] == int(np.sum(rank >= 5))
        tr.eval_forward(x, lab, n_valid=3)  # n_valid below the rows given
        assert tr.eval_metrics()[0] == last3
        assert tr.metrics() == records, "the training records changed"
    finally:
        tr.close()


# ---- 5. training is untouched ----
def _two_steps(track, evaluate):
    from resnet_amd import Trainer
    dims, batch = synth.C1S_DIMS, 4
    tr = Trainer(dims, batch)
    try:
        tr.source_synthetic()
        if track:
            tr.track_running_stats(0.1)
        losses = [tr.step()]
        if evaluate:
            tr.eval_forward()
        losses.append(tr.step())
        assert tr.check_errors() == 0
        tr.check()
        return losses, [tr.get(w, i) for w in ("params", "means", "vars") for i in range(tr.n_locations)], tr.running_updates()
    finally:
        tr.close()


def test_training_is_untouched():
    off, on, ev = _two_steps(False, False), _two_steps(True, False), _two_steps(True, True)
    assert off[2] == 0 and on[2] == 2 and ev[2] == 2
    assert off[0] == on[0] == ev[0]
    for i, (a, b, c) in enumerate(zip(off[1], on[1], ev[1])):
        assert _same(a, b), "tracking on / off: tensor %d of (params, means, vars) differs" % i
        assert _same(b, c), "with / without an eval pass between the steps: tensor %d of (params, means, vars) differs" % i


def _four_steps_and_eval(dtype, first_policy, rebuild_to=None):
    """two steps, (a change of the store policy: every buffer dropped and rebuilt), two more steps, one eval pass with labels"""
    dims, batch = NETS["C4I"]
    tr = _trainer(dims, batch, dtype, first_policy)
    try:
        for step in range(4):
            if step == 2 and rebuild_to is not None:
                tr.set_store_policy(rebuild_to)
            _load(tr, dims, batch, step)
            tr.forward(); tr.backward(); tr.update()
        assert tr.check_errors() == 0
        im, lab = synth.make_batch(dims, batch, step=4)
        tr.eval_forward(T.nhwc_to_nchw(im), lab)
        tr.check()
        rm, rv = tr.running_stats()
        return {"params": [tr.get("params", i) for i in range(tr.n_locations)], "running means": rm, "running vars": rv,
                "updates": tr.running_updates(), "pred": tr.activation("softmax"), "metrics": tr.eval_metrics()}
    finally:
        tr.close()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_the_network_follows_a_rebuild_of_the_buffers(dtype):
    """C4I has every role of a unit (a projection block, an identity block with a block behind it, a striding block) and both
    BN-written channel-last edges.  FAST and RECOMPUTE_BN are bit-identical (test_store_policies_bit_identical_after_25_steps), so a
    trainer that changes policy between steps 2 and 3 must end where one that had the second policy from the start ends -- unless
    something kept from before the rebuild (a cache pointer of the running-statistics table, a plane's writer, a weight-table
    entry) is still read"""
    from resnet_amd import binding as B
    a = _four_steps_and_eval(dtype, B.MI_STORE_FAST, rebuild_to=B.MI_STORE_RECOMPUTE_BN)
    b = _four_steps_and_eval(dtype, B.MI_STORE_RECOMPUTE_BN)
    for i, (x, y) in enumerate(zip(a["params"], b["params"])):
        assert _same(x, y), "parameter tensor %d differs behind the rebuild" % i
    for name in ("running means", "running vars", "pred"):
        assert _same(a[name], b[name]), "%s differ behind the rebuild" % name
    assert a["updates"] == b["updates"] == 4
    assert a["metrics"] == b["metrics"] and a["metrics"][0]["rows"] == NETS["C4I"][1]
    assert np.float64(a["metrics"][0]["loss_sum"]).tobytes() == np.float64(b["metrics"][0]["loss_sum"]).tobytes()


def test_backward_behind_an_eval_pass_is_refused():
    dims, batch = synth.C1S_DIMS, 4
    tr = _trainer(dims, batch)
    try:
        _load(tr, dims, batch, 0)
        tr.forward()
        tr.backward()
        tr.check()
        grads = [tr.get("grads", i) for i in range(tr.n_locations)]
        assert any(np.any(g != 0) for g in grads)
        tr.eval_forward()
        tr.check()
        tr.backward()
        assert "mi_trainer_eval_forward" in tr.error() and "forward_pass" in tr.error()
        tr.L.mi_clear_error()
        for i, g in enumerate(grads):
            assert _same(g, tr.get("grads", i)), "gradient %d changed" % i
        tr.forward()  # a new forward_pass makes backward valid again: the same batch, the same gradients
        tr.backward()
        tr.check()
        for i, g in enumerate(grads):
            assert _same(g, tr.get("grads", i)), "gradient %d after a new forward_pass" % i
    finally:
        tr.close()


def test_sync_bn_with_one_rank_updates_the_same_values():
    """all one GPU can show of sync-BN: with the one-rank communicator the update runs behind the merged statistics and the values
    are those of the plain run (the world factor of the sample count is a host computation: tests/test_eval_model.py)"""
    dims, batch = synth.C1S_DIMS, 4
    res = []
    for sync in (False, True):
        tr = _trainer(dims, batch)
        try:
            if sync:
                nbytes = tr.L.mi_dp_unique_id_bytes()
                ids = [(C.c_char * nbytes)() for _ in range(2)]
                for u in ids:
                    assert tr.L.mi_dp_get_unique_id(u, nbytes) == 0, tr.error()
                assert tr.L.mi_dp_init(tr.t, 0, 1, ids[0], nbytes) == 0, tr.error()
                assert tr.L.mi_dp_enable_sync_bn(tr.t, ids[1], nbytes) == 0, tr.error()
            _load(tr, dims, batch, 0)
            tr.forward()
            tr.check()
            res.append(tr.running_stats() + (tr.running_updates(),))
        finally:
            if sync:
                tr.L.mi_dp_enable_sync_bn(tr.t, None, 0)
            tr.close()
    assert _same(res[0][0], res[1][0]) and _same(res[0][1], res[1][1]) and res[0][2] == res[1][2] == 1


# ---- 6. evaluate_u8 ----
def test_evaluate_u8_is_decode_plus_eval_forward(ops):
    dims, N, dim_in = synth.C1_DIMS, 4, 40
    n = 2 * N + 3
    rng = np.random.RandomState(77)
    images = rng.randint(0, 256, size=(n, dim_in, dim_in, 3)).astype(np.uint8)
    labels = rng.randint(0, dims["output"], size=n).astype(np.int32)
    tr = _trainer(dims, N)
    try:
        _load(tr, dims, N, 0)
        tr.forward()
        tr.check()
        book = lambda: (tr.t.contents.cur_dump_id, tr.c_batch.contents.cur_shard_id, tr.c_batch.contents.cur_batch_in_shard, tr.running_updates())
        before, input_before = book(), tr.activation("input")
        tr.eval_metrics(reset=True)
        for at in range(0, n, N):
            nv = min(N, n - at)
            dec = ops.decode_u8(images[at:at + nv], E.center_plan(nv, dim_in, dims["input"]), dims["input"])
            tr.eval_forward(dec, labels[at:at + nv])
        hand = tr.eval_metrics()[1]
        got = tr.evaluate_u8(images, labels, dim_in, topk=5)
        tr.check()
        assert got["rows"] == n and got["batches"] == 3
        assert np.float64(got["loss_sum"]).tobytes() == np.float64(hand["loss_sum"]).tobytes(), (got, hand)
        assert got == hand
        assert tr.eval_metrics()[1] == got
        assert book() == before and _same(tr.activation("input"), input_before)
        assert tr.evaluate_u8(images, labels, dim_in, topk=5) == got  # the total starts from zero every time
    finally:
        tr.close()


# ---- 7. checkpoint ----
def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_checkpoint_round_trip(tmp_path):
    dims, batch = synth.C1_DIMS, 4
    listing = {}
    for track in (True, False):
        tr = _trainer(dims, batch, track=track, dump_dir="ck")
        try:
            root = str(tmp_path / ("on" if track else "off"))
            tr.L.mi_trainer_set_dump_root(tr.t, root.encode())
            for step in range(2):
                _load(tr, dims, batch, step)
                tr.forward(); tr.backward(); tr.update()
            assert tr.check_errors() == 0
            tr.L.dump_trainer(5, tr.t, b"ck")
            tr.check()
            listing[track] = _files(root)
            if track:
                kept = tr.running_stats(), tr.running_updates()
        finally:
            tr.close()
    name = os.path.join("ck", "%08d" % 5, "bn_running.buffer")
    assert name in listing[True] and [f for f in listing[True] if f != name] == listing[False]
    for f in listing[False]:  # tracking changes no other file
        assert open(str(tmp_path / "on" / f), "rb").read() == open(str(tmp_path / "off" / f), "rb").read(), f
    raw = open(str(tmp_path / "on" / name), "rb").read()
    ch = sum(E.bn_channels(dims))
    assert len(raw) == 2 * ch * 4 + 8 and np.frombuffer(raw[-8:], np.int64)[0] == 2
    assert _same(np.frombuffer(raw[:ch * 4], np.float32), kept[0][0]) and _same(np.frombuffer(raw[ch * 4:2 * ch * 4], np.float32), kept[0][1])
    for track in (True, False):
        tr = _trainer(dims, batch, track=track, dump_dir="ck")
        try:
            tr.L.mi_trainer_set_dump_root(tr.t, str(tmp_path / "on").encode())
            tr.L.overwrite_model_params(tr.t, 5, b"ck")
            tr.check()
            if track:
                rm, rv = tr.running_stats()
                assert _same(rm, kept[0][0]) and _same(rv, kept[0][1]) and tr.running_updates() == kept[1] == 2
            else:
                assert tr.L.mi_trainer_running_stats_channels(tr.t) == 0 and tr.running_updates() == 0
        finally:
            tr.close()


# ---- 8. refusals ----
def _refused(tr, rc, word):
    try:
        assert rc == -1 and word in tr.error(), (rc, tr.error())
    finally:
        tr.L.mi_clear_error()


def test_refusals():
    from resnet_amd import binding as B
    dims, batch = synth.C1_DIMS, 4
    tr = _trainer(dims, batch, track=False)
    L, t = tr.L, tr.t
    try:
        im = C.cast(tr.c_batch.contents.images, C.c_void_p)
        _refused(tr, L.mi_trainer_eval_forward(t, im, None, batch, 1), "not tracked")
        _refused(tr, L.mi_trainer_get_running_stats(t, None, None), "not tracked")
        for m in (0.0, 1.5):
            _refused(tr, L.mi_trainer_track_running_stats(t, 1, m), "momentum lies in (0, 1]")
        assert L.mi_trainer_running_stats_channels(t) == 0
        tr.track_running_stats(1.0)
        ch = L.mi_trainer_running_stats_channels(t)
        assert ch == sum(E.bn_channels(dims))
        for nv in (0, batch + 1):
            _refused(tr, L.mi_trainer_eval_forward(t, im, None, nv, 1), "n_valid lies in [1, batch_size]")
        for k in (0, dims["output"] + 1):
            _refused(tr, L.mi_trainer_eval_forward(t, im, None, batch, k), "topk lies in [1, number of classes]")
        good = np.ones(ch, np.float32)
        for bad_m, bad_v, word in ((np.nan, 1.0, "not finite"), (0.0, np.inf, "not finite"), (0.0, -1e-3, "negative")):
            mm, vv = good.copy(), good.copy()
            mm[ch // 2], vv[ch // 3] = bad_m, bad_v
            _refused(tr, L.mi_trainer_set_running_stats(t, mm.ctypes.data, vv.ctypes.data), word)
        rm, rv = tr.running_stats()
        assert np.all(rm == 0) and np.all(rv == 1), "a refused set wrote something"
        out = B.MiLossMetrics()
        u8 = np.zeros((1, 32, 32, 3), np.uint8)
        _refused(tr, L.mi_trainer_eval_u8(t, u8.ctypes.data, np.zeros(1, np.int32).ctypes.data, 0, 32, 1, C.byref(out)), "n >= 1")
        _refused(tr, L.mi_trainer_eval_u8(t, u8.ctypes.data, np.zeros(1, np.int32).ctypes.data, 1, 31, 1, C.byref(out)), "smaller than the network's input")
        tr.track_running_stats(on=False)
        _refused(tr, L.mi_trainer_eval_forward(t, im, None, batch, 1), "not tracked")
        tr.track_running_stats(0.5)
        tr.set_store_policy(B.MI_STORE_FULL)
        _refused(tr, L.mi_trainer_eval_forward(t, im, None, batch, 1), "FULL store policy")
        _load(tr, dims, batch, 0)
        tr.forward()  # FULL tracks all the same (the table follows the rebuilt caches)
        tr.check()
        assert tr.running_updates() == 1 and _same(tr.running_stats()[0], (np.float32(0.5) * _batch_stats(tr, dims)[0]).astype(np.float32))
    finally:
        tr.close()


# ---- 9. memory hygiene ----
def _hygiene_run(L, debug):
    dims, batch = synth.C1S_DIMS, 5
    if debug:
        assert L.mi_debug_redzone(4096, 0xFF) == 0
        assert L.mi_debug_lds_fill_mode(1, 0xFFFFFFFF) == 0
    try:
        tr = _trainer(dims, batch, BF16)
        try:
            im, lab = _load(tr, dims, batch, 0)
            tr.forward()
            tr.eval_forward(T.nhwc_to_nchw(im), lab)
            tr.check()
            out = list(tr.running_stats()) + [tr.activation("fc_output"), tr.activation("softmax"), np.float64(tr.eval_metrics()[0]["loss_sum"])]
            if debug:
                assert L.mi_debug_redzone_check() == 0, tr.error()
        finally:
            tr.close()
        if debug:
            assert L.mi_debug_redzone_check() == 0, L.mi_last_error()
            live = C.c_size_t(0)
            checked = C.c_size_t(0)
            L.mi_debug_redzone_stats(C.byref(checked), None, C.byref(live))
            assert checked.value > 0
    finally:
        if debug:
            L.mi_debug_lds_fill_mode(0, 0)
            L.mi_debug_redzone(0, 0)
    return out


def test_memory_hygiene(ops):
    plain, debug = _hygiene_run(ops.L, False), _hygiene_run(ops.L, True)
    for i, (a, b) in enumerate(zip(plain, debug)):
        assert np.all(np.isfinite(b)) and _same(np.asarray(a), np.asarray(b)), "output %d differs under red zones + LDS fill" % i
