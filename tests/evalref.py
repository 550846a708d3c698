"""Plain-torch model of evaluation (include/resnet_mi.h, "evaluation"): torch_ref.TorchNet with the running statistics of
torch.nn.BatchNorm2d and an eval forward that normalises with them.

Per BN layer over n = N x H x W samples per channel, momentum m:
  training   y = BN(x) with the batch mean and the BIASED batch variance (torch_ref.bn_train), then
             rm = (1 - m) rm + m mean,  rv = (1 - m) rv + m var n / (n - 1)     (n <= 1: the factor is 1)
  eval       y = (x - rm) / sqrt(rv + eps) gamma + beta
Initial state: rm = 0, rv = 1, no update.  The layers are kept in the order of the running arena: the order of the BN gammas in
locations[] -- the stem, then per block reduction, spatial, expansion, and projection where the block has one (TorchNet.forward runs
its units in exactly that order).  tests/test_eval_model.py pins bn_track / bn_eval against torch.nn.BatchNorm2d itself.
"""
import numpy as np
import torch
import torch.nn.functional as F

from torch_ref import TorchNet


def unbias(n):
    """n / (n - 1) as the host computes it: in double, stored as float32; 1 where n <= 1"""
    return np.float32(float(n) / float(n - 1)) if n > 1 else np.float32(1.0)


def bn_channels(dims):
    """channels of every BN layer in arena order"""
    f = dims["init_conv_filters"]
    out = [f]
    inc, red, ex = f, f, 4 * f
    for b in range(dims["n_conv_blocks"]):
        if dims["is_block_spatial_reduction"][b]:
            red, ex = red * 2, ex * 2
        out += [red, red, ex]
        if inc != ex:
            out.append(ex)
        inc = ex
    return out


def bn_planes(dims):
    """H (= W) of every BN layer's tensor in arena order: samples per channel = batch x H^2"""
    H = dims["input"] // dims["init_conv_stride"]
    out = [H]
    H //= dims["init_maxpool_stride"]
    f = dims["init_conv_filters"]
    inc, ex = f, 4 * f
    for b in range(dims["n_conv_blocks"]):
        stride = 1
        if dims["is_block_spatial_reduction"][b]:
            stride, ex = 2, ex * 2
        out += [H, H // stride, H // stride]
        if inc != ex:
            out.append(H // stride)
        H //= stride
        inc = ex
    return out


def bn_names(dims):
    """Trainer.activation names of every BN layer's cache in arena order ("batch_norms/.../" + "means" | "vars")"""
    out = ["batch_norms/init/"]
    f = dims["init_conv_filters"]
    inc, ex = f, 4 * f
    for b in range(dims["n_conv_blocks"]):
        if dims["is_block_spatial_reduction"][b]:
            ex *= 2
        out += ["batch_norms/%02d/%s/" % (b, leaf) for leaf in ("reduced", "spatial", "expanded")]
        if inc != ex:
            out.append("batch_norms/%02d/projected/" % b)
        inc = ex
    return out


def center_plan(n, dim_in, dim_out):
    """the MI_AUG_CENTER plan of mi_augment_plan: (row_off, col_off, flip) per image"""
    o = (dim_in - dim_out) // 2
    return np.tile(np.array([o, o, 0], np.int32), (n, 1))


def new_state(C, dtype=torch.float64):
    return {"mean": torch.zeros(C, dtype=dtype), "var": torch.ones(C, dtype=dtype), "updates": 0}


def running_update(old_mean, old_var, mean, var_biased, n, m):
    """the update rule on arrays of any float type (float64 numpy in the kernel test)"""
    ub = float(n) / float(n - 1) if n > 1 else 1.0
    return (1 - m) * old_mean + m * mean, (1 - m) * old_var + m * (var_biased * ub)


def bn_track(x, g, b, eps, state, m):
    """training-mode BN of x (NCHW) that also advances `state`"""
    mean = x.mean(dim=(0, 2, 3))
    var = ((x - mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
    n = x.shape[0] * x.shape[2] * x.shape[3]
    state["mean"], state["var"] = running_update(state["mean"], state["var"], mean.detach(), var.detach(), n, m)
    state["updates"] += 1
    return (x - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + eps) * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def bn_eval(x, g, b, eps, state):
    rm, rv = state["mean"].view(1, -1, 1, 1), state["var"].view(1, -1, 1, 1)
    return (x - rm) / torch.sqrt(rv + eps) * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


class EvalNet(TorchNet):
    """TorchNet that tracks running statistics in forward() and normalises with them in eval_forward()"""

    def __init__(self, dims, params, eps=1e-7, dtype=torch.float64, momentum=0.1):
        super().__init__(dims, params, eps, dtype)
        self.momentum = momentum
        self.state = [new_state(C, dtype) for C in bn_channels(dims)]
        self.training = True
        self._layer = 0

    def _unit(self, x, i, K, C, k, stride, relu, name):
        st = self.state[self._layer]
        self._layer += 1
        y = F.conv2d(x, self.p[i].view(K, C, k, k), stride=stride, padding=k // 2)
        y.retain_grad()
        self.acts[name + "_conv"] = y
        if self.training:
            z = bn_track(y, self.p[i + 1], self.p[i + 2], self.eps, st, self.momentum)
        else:
            z = bn_eval(y, self.p[i + 1], self.p[i + 2], self.eps, st)
        if relu:
            z = F.relu(z)
        z.retain_grad()
        self.acts[name] = z
        return z

    def forward(self, images_nchw, labels):
        self._layer, self.training = 0, True
        return super().forward(images_nchw, labels)

    def eval_forward(self, images_nchw):
        """logits (N, output) as a numpy array; the state is not advanced"""
        self._layer = 0
        self.training = False
        try:
            TorchNet.forward(self, images_nchw, np.zeros(len(images_nchw), np.int64))
        finally:
            self.training = True
        return self.acts["logits"].detach().numpy()

    def running(self):
        """(means, vars) packed in arena order, float64"""
        return (np.concatenate([s["mean"].double().numpy() for s in self.state]),
                np.concatenate([s["var"].double().numpy() for s in self.state]))
