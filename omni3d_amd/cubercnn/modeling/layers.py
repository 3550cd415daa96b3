"""nn.Module shells over the HIP kernels.  They subclass the torch modules so that parameter /
buffer names (state-dict keys), `isinstance(m, nn.BatchNorm2d)` checks (solver/build.py:8-19,71-76
of the reference) and `.to(device)` behave exactly like the reference's modules; only `forward`
differs: it launches the gfx950 kernels through omni3d_amd.functional."""
import torch
from torch import nn

from ... import functional as HF

CL = torch.channels_last


class Conv2d(nn.Conv2d):
    """weight (K,C,R,S) held in channels_last memory (= KRSC)."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        assert self.dilation == (1, 1) and self.groups == 1 and self.kernel_size[0] == self.kernel_size[1]
        self.weight.data = self.weight.data.contiguous(memory_format=CL)

    def _load_from_state_dict(self, *a, **k):
        super()._load_from_state_dict(*a, **k)
        self.weight.data = self.weight.data.contiguous(memory_format=CL)

    def forward(self, x, relu=False):
        # a bias-free convolution in training mode is the conv half of a conv -> BatchNorm pair (every one in the DLA / ResNet
        # bottom-up): let the kernel emit the batch statistics with its output -- unless that BatchNorm is frozen (eval mode: freeze_bn)
        # and would not read them.  The BatchNorm makes itself known through the tag on the output (BatchNorm2d._note_producer).
        pair = self.bias is None and self.training and not relu and torch.is_grad_enabled()
        bn = self.__dict__.get("_stats_reader") if pair else None
        y = HF.conv2d(x, self.weight, self.bias, self.stride[0], self.padding[0], relu, pair and (bn is None or bn.training))
        if pair:
            y._omni_stats_producer = self
        return y


class GroupedConv2d(nn.Conv2d):
    """nn.Conv2d(C, K, k, groups=G, bias=False) (DLA BottleneckX): weight (K, C/G, k, k) in channels_last memory.  The kernels move
    4 channels per lane: groups narrower than that (the 2 -> 2 channel groups of dla46x_c / dla60x_c) are zero-padded to 4 input and
    4 output channels per group around the call (index permutations and pads in torch, the convolution itself on the same kernels)."""

    def __init__(self, cin, cout, kernel_size, stride=1, padding=0, groups=1):
        super().__init__(cin, cout, kernel_size, stride=stride, padding=padding, groups=groups, bias=False)
        self.weight.data = self.weight.data.contiguous(memory_format=CL)

    def _load_from_state_dict(self, *a, **k):
        super()._load_from_state_dict(*a, **k)
        self.weight.data = self.weight.data.contiguous(memory_format=CL)

    def forward(self, x):
        G, cg, kg = self.groups, self.in_channels // self.groups, self.out_channels // self.groups
        if cg % 4 == 0 and kg % 4 == 0:
            return HF.grouped_conv2d(x, self.weight, G, self.stride[0], self.padding[0])
        import torch.nn.functional as F
        c4, k4 = (cg + 3) // 4 * 4, (kg + 3) // 4 * 4
        n, _, h, w = x.shape
        xp = F.pad(x.reshape(n, G, cg, h, w), (0, 0, 0, 0, 0, c4 - cg)).reshape(n, G * c4, h, w)
        r = self.kernel_size[0]
        wp = F.pad(self.weight.reshape(G, kg, cg, r, r), (0, 0, 0, 0, 0, c4 - cg, 0, k4 - kg)).reshape(G * k4, c4, r, r)
        y = HF.grouped_conv2d(xp.contiguous(memory_format=CL), wp.contiguous(memory_format=CL), G, self.stride[0], self.padding[0])
        return y.reshape(n, G, k4, y.shape[2], y.shape[3])[:, :, :kg].reshape(n, G * kg, y.shape[2], y.shape[3])


class DepthwiseConv2d(nn.Conv2d):
    """nn.Conv2d(C, C, k, groups=C, bias=False) (torchvision mnasnet) on csrc/depthwise.hip; weight (C, 1, k, k)"""

    def __init__(self, channels, kernel_size, stride=1, padding=0):
        super().__init__(channels, channels, kernel_size, stride=stride, padding=padding, groups=channels, bias=False)
        assert kernel_size in (3, 5) and stride in (1, 2)

    def forward(self, x):
        return HF.depthwise_conv2d(x, self.weight, self.stride[0], self.padding[0])


class Linear(nn.Linear):
    def forward(self, x, relu=False):
        return HF.linear(x, self.weight, self.bias, relu)


class FlattenLinear(nn.Module):
    """`flatten -> nn.Linear(C*P*P, out)` of FastRCNNConvFCHead / CubeHead fc1, computed as a PxP
    valid convolution over the NHWC ROI features.  The parameter is kept (out, C, P, P) in
    channels_last memory so the GEMM reduction index is contiguous; state dicts carry the
    reference's (out, C*P*P) shape."""

    def __init__(self, channels, size, out_features):
        super().__init__()
        self.channels, self.size, self.out_features = channels, size, out_features
        w = torch.empty(out_features, channels, size, size)
        nn.init.kaiming_uniform_(w, a=1)  # c2_xavier_fill
        self.weight = nn.Parameter(w.contiguous(memory_format=CL))
        self.bias = nn.Parameter(torch.zeros(out_features))
        self._register_state_dict_hook(self._to_reference_shape)
        self._register_load_state_dict_pre_hook(self._from_reference_shape)

    @staticmethod
    def _to_reference_shape(module, state_dict, prefix, local_metadata):
        key = prefix + "weight"
        state_dict[key] = state_dict[key].reshape(module.out_features, -1)

    def _from_reference_shape(self, state_dict, prefix, *args):
        key = prefix + "weight"
        if key in state_dict and state_dict[key].dim() == 2:
            state_dict[key] = state_dict[key].reshape(self.out_features, self.channels, self.size, self.size)

    def forward(self, x, relu=False):
        """x: (R, C, P, P) channels_last (physically (R, P, P, C)) -> (R, out).  With KRSC weights the
        flattened (p, p, c) order is contiguous on both operands, so this is a plain GEMM (forward,
        dgrad and wgrad) on 2-D views -- no im2col gather."""
        R = x.shape[0]
        x2 = x.permute(0, 2, 3, 1).reshape(R, -1)
        w2 = self.weight.permute(0, 2, 3, 1).reshape(self.out_features, -1)
        gview = None
        if getattr(self.weight, "_omni_direct_grad", False) and self.weight.grad is not None:
            gview = self.weight.grad.permute(0, 2, 3, 1).reshape(self.out_features, -1)
            w2 = w2.detach().requires_grad_(True) if False else w2
        return HF.linear(x2, w2, self.bias, relu, gview)


PARAM_EPOCH = [0]        # bumped by every parameter update torch's version counters do not see (solver/build.py FlatOptimizer.step)
BN_MODE_EPOCH = [0]      # bumped whenever a BatchNorm2d's `training` or `track_running_stats` changes (freeze_bn, .train() / .eval())
TRAIN_PASS = [0]         # > 0 inside a training-mode pass of a model (training_pass): its eval-mode BatchNorms are frozen ones with gradients


class training_pass:
    """Marks the forward pass of a model in training mode (RCNN3D._forward).  An eval-mode BatchNorm2d inside it -- freeze_bn,
    MODEL.USE_BN False -- normalises with its running statistics AND passes gradients (functional.batch_norm_frozen); outside it an
    eval-mode BatchNorm2d is an inference layer and keeps its cached (scale, shift) path, bit for bit (the frozen kernel makes its
    coefficients with the device library's rsqrtf, which differs from torch's GPU rsqrt in the last bit for some values)."""

    def __enter__(self):
        TRAIN_PASS[0] += 1
        return self

    def __exit__(self, *exc):
        TRAIN_PASS[0] -= 1


def frozen_bn_wants_grad(x, bn):
    """an eval-mode BatchNorm of a training pass whose input or affine parameters need a gradient"""
    return TRAIN_PASS[0] > 0 and torch.is_grad_enabled() and (x.requires_grad or bn.weight.requires_grad or bn.bias.requires_grad)


class BatchNorm2d(nn.BatchNorm2d):
    # RCNN3D sets this and bumps every `num_batches_tracked` of the model with ONE multi-tensor add per step
    defer_counter = False

    def __setattr__(self, name, value):
        # a captured training step holds the kernels of one BatchNorm mode (batch statistics or frozen): solver/autoreplay.py watches this
        if name in ("training", "track_running_stats") and self.__dict__.get(name, value) != value:
            BN_MODE_EPOCH[0] += 1
        super().__setattr__(name, value)

    def _note_producer(self, x):
        """the bias-free Conv2d that wrote x learns which BatchNorm reads its output (Conv2d.forward: no batch statistics for a frozen one)"""
        conv = getattr(x, "_omni_stats_producer", None)
        if conv is not None and conv.__dict__.get("_stats_reader") is not self:
            conv.__dict__["_stats_reader"] = self          # (not a submodule: kept out of nn.Module's registry)

    def forward(self, x, residual=None, relu=False):
        if self.training:
            self._note_producer(x)
            y = HF.batch_norm_train(x, self.weight, self.bias, self.running_mean if self.track_running_stats else None,
                                    self.running_var if self.track_running_stats else None, residual, relu, self.eps,
                                    self.momentum)
            if self.track_running_stats and self.num_batches_tracked is not None and not self.defer_counter:
                self.num_batches_tracked += 1
            if self.track_running_stats:
                PARAM_EPOCH[0] += 1          # the kernel moved the running statistics through raw pointers: eval-mode caches are stale
            return y
        if frozen_bn_wants_grad(x, self):
            # frozen BatchNorm of a training pass (freeze_bn, MODEL.USE_BN False): the running statistics normalise, gamma / beta and
            # everything below get gradients.  (scale, shift) are made inside the kernel from the live tensors: nothing a captured
            # graph could hold stale
            self._note_producer(x)
            return HF.batch_norm_frozen(x, self.weight, self.bias, self.running_mean, self.running_var, residual, relu, self.eps)
        from ...kernels import bnpool
        # inference: (scale, shift) of the frozen statistics, built once per set of values (six ATen launches per layer and call
        # otherwise: 234 of the 805 launches of an inference pass, profiles/r04_infer_trace_table.txt).  The key catches every write
        # torch knows about (load_state_dict, copy_, in-place ops bump `_version`) and PARAM_EPOCH the ones it cannot see (the flat
        # optimizers update parameters through raw pointers: FlatOptimizer.step bumps it)
        key = (PARAM_EPOCH[0], self.weight._version, self.bias._version, self.running_mean._version, self.running_var._version,
               self.weight.data_ptr(), self.running_var.data_ptr())
        cached = self.__dict__.get("_eval_scale_shift")
        if cached is None or cached[0] != key:
            with torch.no_grad():
                scale = self.weight * torch.rsqrt(self.running_var + self.eps)
                cached = (key, torch.cat([scale, self.bias - self.running_mean * scale]).contiguous())
            self.__dict__["_eval_scale_shift"] = cached
        scale_shift = cached[1]
        return bnpool.bn_apply(x.contiguous(memory_format=CL), scale_shift,
                               residual.contiguous(memory_format=CL) if residual is not None else None, relu)
