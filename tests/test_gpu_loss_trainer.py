"""The trainer's loss head (mi_trainer_set_loss / mi_trainer_metrics, include/resnet_mi.h) on C1S at batch 8, host source.

  DEVICE, eps 0        three steps against a trainer on the default path fed the same batches: parameters, Adam moments and pred bit for bit,
                       wrong_top1 = mi_host_loss's count, loss_sum within the summed per-row bound of -log of the host's pred, the totals
  DEVICE | NO_PRED_COPY  the same parameters, mi_host_loss answers from the device's record, pred_cpu is left alone
  eps 0.1              one step against torch's label-smoothed cross entropy on the float64 network (and eps 0 through the same subclass)
  bf16 storage         DEVICE, eps 0 == the bf16 default path bit for bit
  launches             the default path launches softmax_kernel and ce_deriv_kernel, DEVICE loss_head_kernel and neither of the two
  flag rules           every refused combination returns -1 with a message
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lossref as R
import synth
import torch_ref
from util import GRAD_REL_L2, LOSS_ABS, check_grad

pytestmark = pytest.mark.gpu

DIMS, BATCH, STEPS = synth.C1S_DIMS, 8, 3
HOST, DEVICE, NO_PRED_COPY = 0, 1, 2
SENTINEL = np.float32(-7.0)  # no probability


@pytest.fixture(scope="module")
def params():
    return synth.make_params(DIMS, perturb_bn=True)


def _trainer(params, dtype=0):
    from resnet_amd import Trainer
    from resnet_amd import binding as B
    tr = Trainer(DIMS, BATCH)
    if tr.L.mi_device_count() < 1:
        pytest.fail("no HIP device: this test must run on the MI355X box")
    tr.set_dtype(dtype)
    tr.set_params(params)
    tr.source_host(B.MI_LAYOUT_NHWC)
    return tr


def _load(tr, step):
    im, lab = synth.make_batch(DIMS, BATCH, step=step)
    tr.fill_host_batch(im, lab)
    tr.load_new_batch()
    return im, lab


def _pred_cpu(tr):
    return np.ctypeslib.as_array(tr.t.contents.forward_buffer.contents.pred_cpu, shape=(BATCH * DIMS["output"],))


def _steps(params, smoothing, topk, flags, dtype=0, steps=STEPS):
    """per step: mi_host_loss, pred (device), pred_cpu, labels, the two records, then parameters and Adam moments after the update"""
    tr = _trainer(params, dtype)
    out = []
    try:
        assert tr.L.mi_trainer_set_loss(tr.t, smoothing, topk, flags) == 0, tr.error()
        _pred_cpu(tr)[:] = SENTINEL
        for s in range(steps):
            _, lab = _load(tr, s)
            tr.forward()
            tr.check()
            rec = {"loss": tr.loss(), "pred": tr.activation("softmax"), "pred_cpu": tr.pred(), "labels": lab}
            rec["last"], rec["total"] = tr.metrics()
            tr.backward()
            tr.update()
            assert tr.check_errors() == 0
            rec["state"] = [tr.get(w, i) for w in ("params", "means", "vars") for i in range(tr.n_locations)]
            out.append(rec)
        last, total = tr.metrics(reset=True)
        assert total == out[-1]["total"] and last == out[-1]["last"]
        assert all(v == 0 for v in tr.metrics()[1].values())  # reset_total zeroed it
    finally:
        tr.close()
    return out


@pytest.fixture(scope="module")
def default_run(params):
    return _steps(params, 0.0, 1, HOST)


@pytest.fixture(scope="module")
def device_run(params):
    return _steps(params, 0.0, 5, DEVICE)


def _same_state(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "%s: tensor %d of (params, means, vars) differs" % (what, i)


def test_device_head_equals_the_default_path(default_run, device_run):
    zero = {"loss_sum": 0.0, "rows": 0, "wrong_top1": 0, "wrong_topk": 0, "batches": 0}
    running = 0.0
    for s, (d, g) in enumerate(zip(default_run, device_run)):
        _same_state(d["state"], g["state"], "step %d" % s)
        assert np.array_equal(d["pred"].view(np.uint32), g["pred"].view(np.uint32))
        assert np.array_equal(d["pred_cpu"].view(np.uint32), g["pred_cpu"].view(np.uint32))
        assert np.array_equal(g["pred_cpu"], g["pred"])
        assert g["loss"] == d["loss"]  # the copy stayed: mi_host_loss on pred_cpu, as before
        assert d["last"] == zero and d["total"] == zero
        last, lab = g["last"], g["labels"]
        assert last["wrong_top1"] == d["loss"][1] and last["rows"] == BATCH and last["batches"] == 1
        assert last["wrong_topk"] == int(np.sum(R.rank_of(g["pred"], lab) >= 5))
        rows = -np.log(d["pred_cpu"].astype(np.float64)[np.arange(BATCH), lab])
        assert abs(last["loss_sum"] - rows.sum()) <= R.loss_bound(rows).sum(), (s, last["loss_sum"], rows.sum())
        running += last["loss_sum"]
        tot = g["total"]
        assert tot["loss_sum"] == running and tot["batches"] == s + 1 and tot["rows"] == (s + 1) * BATCH
        assert tot["wrong_top1"] == sum(r["last"]["wrong_top1"] for r in device_run[:s + 1])
        assert tot["wrong_topk"] == sum(r["last"]["wrong_topk"] for r in device_run[:s + 1])


def test_no_pred_copy(params, device_run):
    run = _steps(params, 0.0, 5, DEVICE | NO_PRED_COPY)
    for s, (g, n) in enumerate(zip(device_run, run)):
        _same_state(g["state"], n["state"], "step %d" % s)
        assert np.array_equal(g["pred"].view(np.uint32), n["pred"].view(np.uint32))
        assert n["last"] == g["last"] and n["total"] == g["total"]
        assert n["loss"] == (float(np.float32(n["last"]["loss_sum"])), n["last"]["wrong_top1"])
        assert np.all(n["pred_cpu"] == SENTINEL)  # what it held before the first forward_pass


class SmoothedNet(torch_ref.TorchNet):
    """the float64 network with torch's label-smoothed cross entropy, a batch SUM, in place of its -log p_c"""

    def __init__(self, dims, params, smoothing):
        super().__init__(dims, params)
        self.smoothing = smoothing

    def forward(self, images_nchw, labels):
        super().forward(images_nchw, labels)
        lab = torch.tensor(np.asarray(labels), dtype=torch.long)
        self.loss = F.cross_entropy(self.acts["logits"], lab, label_smoothing=self.smoothing, reduction="sum")
        return self.loss


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_label_smoothing_against_torch(params, eps):
    im, lab = synth.make_batch(DIMS, BATCH, step=0)
    net = SmoothedNet(DIMS, params, eps)
    ref_loss = float(net.forward(torch_ref.nhwc_to_nchw(im), lab).detach())
    ref_grads = net.backward()
    tr = _trainer(params)
    try:
        tr.set_loss(smoothing=eps, topk=5, device=True)
        _load(tr, 0)
        tr.forward()
        last, _ = tr.metrics()
        tr.backward()
        tr.check()
        print("eps %g: loss %.9g, float64 network %.9g" % (eps, last["loss_sum"], ref_loss))
        assert abs(last["loss_sum"] - ref_loss) <= LOSS_ABS * BATCH, (last["loss_sum"], ref_loss)
        for i in range(tr.n_locations):
            check_grad(tr.get("grads", i), ref_grads[i].reshape(-1), "eps %g: gradient of tensor %d" % (eps, i), GRAD_REL_L2)
    finally:
        tr.close()


def test_bf16_storage(params):
    from resnet_amd import binding as B
    d = _steps(params, 0.0, 1, HOST, B.MI_DTYPE_BF16, steps=1)[0]
    g = _steps(params, 0.0, 5, DEVICE, B.MI_DTYPE_BF16, steps=1)[0]
    _same_state(d["state"], g["state"], "bf16")
    assert np.array_equal(d["pred"].view(np.uint32), g["pred"].view(np.uint32))
    assert g["last"]["wrong_top1"] == d["loss"][1] and g["last"]["rows"] == BATCH


def _ring(L):
    buf = C.create_string_buffer(1 << 16)
    n = L.mi_debug_trace_names(buf, len(buf))
    names = buf.value.decode().split("\n")[:-1]
    assert 0 < n == len(names) < 96, "the launch ring is off, or full (%d): launches were lost" % n
    return names


@pytest.mark.parametrize("flags", [HOST, DEVICE])
def test_launches(params, flags):
    """forward_pass and backwards_pass looked at separately: each fits the ring (the cross-entropy derivative is the first launch of
    backwards_pass)"""
    tr = _trainer(params)
    try:
        assert tr.L.mi_trainer_set_loss(tr.t, 0.0, 1 if flags == HOST else 5, flags) == 0, tr.error()
        _load(tr, 0)
        tr.L.mi_debug_trace_clear()
        tr.forward()
        fwd = _ring(tr.L)
        tr.L.mi_debug_trace_clear()
        tr.backward()
        bwd = _ring(tr.L)
        tr.update()
        assert tr.check_errors() == 0
    finally:
        tr.close()
    heads = [n for n in fwd + bwd if n.startswith(("softmax_kernel", "ce_deriv_kernel", "loss_head_kernel", "loss_reduce_kernel"))]
    if flags == HOST:
        assert heads == ["softmax_kernel", "ce_deriv_kernel"] and fwd[-1] == "softmax_kernel" and bwd[0] == "ce_deriv_kernel"
    else:
        assert heads == ["loss_head_kernel<reg>", "loss_reduce_kernel"] and fwd[-2:] == heads


def test_flag_rules(params):
    tr = _trainer(params)
    L = DIMS["output"]
    try:
        for smoothing, topk, flags, word in ((0.1, 5, HOST, "MI_LOSS_DEVICE"), (0.0, 5, NO_PRED_COPY, "MI_LOSS_DEVICE"), (0.1, 5, NO_PRED_COPY, "MI_LOSS_DEVICE"),
                                             (1.0, 5, DEVICE, "smoothing"), (-0.5, 5, DEVICE, "smoothing"), (0.1, 0, DEVICE, "topk"),
                                             (0.1, L + 1, DEVICE, "topk"), (0.0, 1, 4, "flag")):
            assert tr.L.mi_trainer_set_loss(tr.t, smoothing, topk, flags) == -1, (smoothing, topk, flags)
            msg = tr.error()
            tr.L.mi_clear_error()
            assert "mi_trainer_set_loss" in msg and word in msg, msg
        with pytest.raises(RuntimeError):
            tr.set_loss(smoothing=0.1, device=False)
        # a refused call leaves the default head in place; the setting may change between steps
        _load(tr, 0); tr.forward(); host = tr.loss(); tr.backward(); tr.update()
        assert all(v == 0 for v in tr.metrics()[0].values())
        tr.set_loss(smoothing=0.0, topk=L, device=True, copy_pred=False)
        _load(tr, 1); tr.forward(); dev = tr.loss(); tr.backward(); tr.update()
        assert tr.check_errors() == 0
        last, _ = tr.metrics()
        assert last["batches"] == 1 and last["wrong_topk"] == 0 and dev == (float(np.float32(last["loss_sum"])), last["wrong_top1"])
        assert np.isfinite(host[0]) and np.isfinite(dev[0])
    finally:
        tr.close()
