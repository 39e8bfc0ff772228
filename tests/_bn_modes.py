"""Shared by the BatchNorm-mode tests (tests/test_bn_modes_cpu.py, tests/test_gpu_bn_modes.py): a plain-torch fp64 forward of
a TactileSR built from the module's OWN ``nn.Conv2d`` / ``nn.BatchNorm2d`` children on the CPU (``F.interpolate``,
``F.conv2d``, ``F.batch_norm``) that honours each BatchNorm layer's ``training`` flag -- the oracle has one global
``training`` switch, so it cannot speak for a model whose layers are in different modes.  ReLUs go through an
``oracle.ReluTap`` under the oracle's names, so the GPU tests evaluate the fp64 gradient on the device's own pattern as
tests/_gradcheck.py does.  tests/test_bn_modes_cpu.py pins this helper against the oracle where the oracle can speak (all
layers training, all layers held).  Host only."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import tactilesr_oracle as O


def bn_paths(model):
    """Module paths of every nn.BatchNorm2d of `model`, in registration order."""
    return [n for n, m in model.named_modules() if isinstance(m, nn.BatchNorm2d)]


def trunk_bn_paths(model):
    """The BatchNorm layers of the two containers the Seqs trainer transplants (only the MSRBs have any)."""
    return [n for n in bn_paths(model) if n.startswith(("patternFeatureExtra_layer.", "forceFeatureExtra_layer."))]


def set_modes(model, held):
    """model.train(), then eval mode on exactly the BatchNorm layers whose path is in `held`."""
    model.train()
    mods = dict(model.named_modules())
    assert set(held) <= set(bn_paths(model)), sorted(set(held) - set(bn_paths(model)))
    for n in held:
        mods[n].eval()
    return model


# the hold patterns of the whole-step tests: name -> BatchNorm paths held
def pattern_paths(model, name):
    if name == "none":
        return []
    if name == "all":
        return bn_paths(model)
    if name == "seqs":          # both trunk containers (the test also freezes their parameters)
        return trunk_bn_paths(model)
    if name == "mixed":         # inside one MSRB: one layer of each shared / sibling launch held, its partner training
        return ["patternFeatureExtra_layer.0.conv_3_1.1", "patternFeatureExtra_layer.0.conv_5_2.1"]
    if name == "stem":          # only stem layer .2 of frame 1
        return ["inputLayer_pattern_list.1.2"]
    raise KeyError(name)


class _Net:
    """One fp64 forward over the module tree of a CPU TactileSR with the parameters in `leaves` (name -> tensor)."""

    def __init__(self, model, leaves, dtype, tap, new_stats):
        self.mods = dict(model.named_modules())
        self.p, self.dtype, self.tap, self.ns = leaves, dtype, tap, new_stats

    def relu(self, name, x):
        return F.relu(x) if self.tap is None else self.tap(name, x)

    def conv(self, path, x):
        m = self.mods[path]
        assert isinstance(m, nn.Conv2d) and m.stride == (1, 1) and m.dilation == (1, 1) and m.groups == 1
        return F.conv2d(x, self.p[path + ".weight"], self.p.get(path + ".bias"), padding=m.padding)

    def bn(self, path, x):
        m = self.mods[path]
        assert isinstance(m, nn.BatchNorm2d) and m.track_running_stats and m.momentum is not None
        rm, rv = m.running_mean.detach().to(self.dtype).clone(), m.running_var.detach().to(self.dtype).clone()
        y = F.batch_norm(x, rm, rv, self.p[path + ".weight"], self.p[path + ".bias"], m.training, m.momentum, m.eps)
        if m.training and self.ns is not None:          # (a held layer writes nothing: it is absent from new_stats)
            self.ns[path + ".running_mean"], self.ns[path + ".running_var"] = rm, rv
            self.ns[path + ".num_batches_tracked"] = m.num_batches_tracked.detach() + 1
        return y

    def conv_bn_relu(self, cpath, bpath, x):
        return self.relu(bpath, self.bn(bpath, self.conv(cpath, x)))

    def msrb(self, p, x):
        o31 = self.conv_bn_relu(p + ".conv_3_1.0", p + ".conv_3_1.1", x)
        o51 = self.conv_bn_relu(p + ".conv_5_1.0", p + ".conv_5_1.1", x)
        in2 = torch.cat([o31, o51], 1)
        o32 = self.conv_bn_relu(p + ".conv_3_2.0", p + ".conv_3_2.1", in2)
        o52 = self.conv_bn_relu(p + ".conv_5_2.0", p + ".conv_5_2.1", in2)
        return self.relu(p + ".out", self.conv(p + ".confusion", torch.cat([o32, o52], 1)) + x)

    def res(self, p, x):
        y = self.relu(p + ".conv1", self.conv(p + ".conv1", x))
        return self.relu(p + ".out", x + self.conv(p + ".conv2", y))


def forward(model, x, leaves=None, dtype=torch.float64, tap=None, new_stats=None):
    """TactileSR.forward (reference model/tactileSR_model.py:67-84) of the CPU module `model` in `dtype`, every BatchNorm
    layer in ITS OWN mode.  `leaves` (name -> tensor) replaces the parameters (the gradient leaves)."""
    if leaves is None:
        leaves = {n: p.detach().to(dtype) for n, p in model.named_parameters()}
    net = _Net(model, leaves, dtype, tap, new_stats)
    sf, A = model.scale_factor, model.axisCnt
    x = x.to(dtype)
    size = (x.shape[2] * sf, x.shape[3] * sf)
    feats = []
    for t in range(model.seqsCnt):
        pre = f"inputLayer_pattern_list.{t}"
        u = F.interpolate(x[:, A * t:A * (t + 1)], size=size, mode="bilinear", align_corners=False)
        h = net.conv_bn_relu(pre + ".1", pre + ".2", u)
        feats.append(net.conv_bn_relu(pre + ".4", pre + ".5", h))
    h = torch.cat(feats, 1)
    h = net.conv_bn_relu("inputContact_layer.0", "inputContact_layer.1", h)
    for i in range(len(model.patternFeatureExtra_layer)):
        h = net.msrb(f"patternFeatureExtra_layer.{i}", h)
    u = F.interpolate(x[:, :A], size=size, mode="bilinear", align_corners=False)
    f = net.relu("force_in", net.conv("input_layer_force.1", u))
    for i in range(len(model.forceFeatureExtra_layer)):
        f = net.res(f"forceFeatureExtra_layer.{i}", f)
    out = net.relu("head0", net.conv("output_layer.0", torch.cat((f, h), 1)))
    out = net.relu("out", net.conv("output_layer.2", out))
    return F.interpolate(out, size=(4 * sf, 4 * sf), mode="bilinear", align_corners=False)


def step(model, LR, HR, masks=None, record=False, want_dx=False, dtype=torch.float64):
    """loss, {parameter: gradient}, the new statistics of the TRAINING layers, the ReLU pre-activations (with `record`) and
    (with `want_dx`) the taxel gradient of one forward + backward, the ReLU pattern optionally forced to `masks`: what
    tests/_gradcheck.oracle_grads returns, for per-layer modes."""
    leaves = {n: p.detach().to(dtype).requires_grad_(True) for n, p in model.named_parameters()}
    x = LR.detach().to(dtype).requires_grad_(want_dx)
    tap = O.ReluTap(masks=masks, record=record) if (masks is not None or record) else None
    ns = {}
    out = forward(model, x, leaves, dtype, tap, ns)
    loss = F.mse_loss(out, HR.to(dtype))
    gl = torch.autograd.grad(loss, list(leaves.values()) + ([x] if want_dx else []))
    grads = dict(zip(leaves, gl))
    return float(loss.detach()), grads, ns, (tap.pre if tap is not None else None), (gl[-1] if want_dx else None)
