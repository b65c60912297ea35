"""EfficientNet-B0..B3 with the module tree / state-dict names of torchvision.models.efficientnet (the last alternative backbone of the
reference's feature-extractor configs, configs/dog_fe/fe_dogs_config.py:105-106: `efficientnet_b2(pretrained=True)` with
`classifier = Linear(1408, 512)`).

Restated from the torchvision definition: 3x3 stride-2 stem (Conv → BatchNorm → SiLU), seven stages of MBConv blocks (1x1 expand →
BN → SiLU unless the ratio is 1, depthwise k x k stride s → BN → SiLU, squeeze-and-excitation with max(1, input // 4) squeeze
channels, 1x1 project → BN, "row" stochastic depth and the residual when stride 1 and input == output), a last 1x1 conv → BN → SiLU to
4 x the last stage width, avgpool → Dropout → Linear.  BatchNorm eps 1e-5 / momentum 0.1 (the V1 defaults).  CPU tensors run these
torch layers; CUDA (HIP) tensors run the gfx950 kernels through models/_efficientnet_engine.EfficientNetEngine (depthwise k x k in
csrc/pfr_dwconvk.hip, squeeze-and-excitation in csrc/pfr_se.hip, the SiLU forms of the BatchNorm kernels).
"""
import math

import torch
import torch.nn as nn

from .mobilenet import _make_divisible
from .resnet import _no_pretrained

# expand ratio, kernel, stride, input channels, output channels, layers (width 1.0, depth 1.0 = B0)
_BASE = [(1, 3, 1, 32, 16, 1), (6, 3, 2, 16, 24, 2), (6, 5, 2, 24, 40, 2), (6, 3, 2, 40, 80, 3), (6, 5, 1, 80, 112, 3),
         (6, 5, 2, 112, 192, 4), (6, 3, 1, 192, 320, 1)]


def _scaled_setting(width_mult, depth_mult):
    return [(t, k, s, _make_divisible(ci * width_mult, 8), _make_divisible(co * width_mult, 8), int(math.ceil(n * depth_mult)))
            for t, k, s, ci, co, n in _BASE]


def _conv_bn_silu(inp, oup, kernel_size=3, stride=1, groups=1, act=True):
    """torchvision's Conv2dNormActivation(norm_layer=BatchNorm2d, activation_layer=SiLU | None): keys 0.weight, 1.*"""
    layers = [nn.Conv2d(inp, oup, kernel_size, stride, (kernel_size - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(oup)]
    if act:
        layers.append(nn.SiLU(inplace=True))
    return nn.Sequential(*layers)


class SqueezeExcitation(nn.Module):
    """torchvision.ops.misc.SqueezeExcitation(input_channels, squeeze_channels, activation=SiLU, scale_activation=Sigmoid)"""

    def __init__(self, input_channels, squeeze_channels):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(input_channels, squeeze_channels, 1)
        self.fc2 = nn.Conv2d(squeeze_channels, input_channels, 1)
        self.activation = nn.SiLU(inplace=True)
        self.scale_activation = nn.Sigmoid()

    def forward(self, x):
        scale = self.scale_activation(self.fc2(self.activation(self.fc1(self.avgpool(x)))))
        return scale * x


class MBConv(nn.Module):
    def __init__(self, expand_ratio, kernel, stride, input_channels, out_channels, sd_prob):
        super().__init__()
        if stride not in (1, 2):
            raise ValueError("illegal stride value")
        self.stride, self.kernel = stride, kernel
        self.use_res_connect = stride == 1 and input_channels == out_channels
        expanded = _make_divisible(input_channels * expand_ratio, 8)
        layers = []
        if expanded != input_channels:
            layers.append(_conv_bn_silu(input_channels, expanded, kernel_size=1))
        layers.append(_conv_bn_silu(expanded, expanded, kernel_size=kernel, stride=stride, groups=expanded))
        layers.append(SqueezeExcitation(expanded, max(1, input_channels // 4)))
        layers.append(_conv_bn_silu(expanded, out_channels, kernel_size=1, act=False))
        self.block = nn.Sequential(*layers)
        self.sd_prob = float(sd_prob)   # stochastic depth, mode "row": a whole sample's branch is dropped with this probability
        self.out_channels = out_channels

    def forward(self, x, sd=None):
        """sd: this block's row of EfficientNet._draw_sd (fp32 [N]: 0 or 1/(1-p)), None = keep every sample unscaled"""
        r = self.block(x)
        if not self.use_res_connect:
            return r
        if sd is not None:
            r = r * sd.view(-1, 1, 1, 1).to(r.dtype)
        return x + r


class EfficientNet(nn.Module):
    def __init__(self, inverted_residual_setting=None, dropout=0.2, stochastic_depth_prob=0.2, num_classes=1000, last_channel=None,
                 width_mult=1.0, depth_mult=1.0, compute_dtype=None):
        super().__init__()
        if inverted_residual_setting is None:
            inverted_residual_setting = _scaled_setting(width_mult, depth_mult)
        if len(inverted_residual_setting) == 0 or any(len(c) != 6 for c in inverted_residual_setting):
            raise ValueError("inverted_residual_setting should be a non-empty list of (expand, kernel, stride, in, out, layers)")
        self.stochastic_depth_prob = float(stochastic_depth_prob)
        first = inverted_residual_setting[0][3]
        features = [_conv_bn_silu(3, first, kernel_size=3, stride=2)]
        total = sum(c[5] for c in inverted_residual_setting)
        bid = 0
        self.sd_probs = []
        for t, k, s, ci, co, n in inverted_residual_setting:
            stage = []
            for i in range(n):
                p = self.stochastic_depth_prob * float(bid) / total
                stage.append(MBConv(t, k, s if i == 0 else 1, ci if i == 0 else co, co, p))
                self.sd_probs.append(p)
                bid += 1
            features.append(nn.Sequential(*stage))
        last_in = inverted_residual_setting[-1][4]
        self.last_channel = last_channel if last_channel is not None else 4 * last_in
        features.append(_conv_bn_silu(last_in, self.last_channel, kernel_size=1))
        self.features = nn.Sequential(*features)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(nn.Dropout(p=dropout, inplace=True), nn.Linear(self.last_channel, num_classes))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                r = 1.0 / math.sqrt(m.out_features)
                nn.init.uniform_(m.weight, -r, r)
                nn.init.zeros_(m.bias)
        self.compute_dtype = compute_dtype   # HIP compute dtype: torch.bfloat16 / torch.float32 (None → PFR_COMPUTE_DTYPE / bf16)
        self._engine = None
        self._sd_p = {}

    def blocks(self):
        return [b for st in self.features if isinstance(st[0], MBConv) for b in st]

    def _draw_sd(self, N, device):
        """The stochastic-depth draws of one forward pass: fp32 [n_blocks, N] of 0 or 1/(1-p_b) (torchvision's
        StochasticDepth(p_b, "row") noise); all ones in eval mode or with stochastic_depth_prob = 0."""
        if not self.training or self.stochastic_depth_prob == 0.0:
            return torch.ones(len(self.sd_probs), N, dtype=torch.float32, device=device)
        key = str(device)
        p = self._sd_p.get(key)
        if p is None:
            p = self._sd_p[key] = torch.tensor(self.sd_probs, dtype=torch.float32, device=device)
        keep = (torch.rand(len(self.sd_probs), N, device=device) >= p[:, None]).float()
        return keep / (1.0 - p)[:, None]

    def _forward_torch(self, x, sd):
        bid = 0
        for st in self.features:
            if isinstance(st[0], MBConv):
                for blk in st:
                    x = blk(x, sd[bid])
                    bid += 1
            else:
                x = st(x)
        return self.classifier(torch.flatten(self.avgpool(x), 1))

    def hip_engine(self, device=None):
        from ._efficientnet_engine import EfficientNetEngine
        if self._engine is None or not self._engine.matches(self):
            self._engine = EfficientNetEngine(self, device or next(self.parameters()).device, self.compute_dtype)
        return self._engine

    def forward(self, x, sd=None):
        """sd: the stochastic-depth draw of this pass ([n_blocks, N] of 0 or 1/(1-p_b)); None draws one (_draw_sd)"""
        if sd is None:
            sd = self._draw_sd(x.shape[0], x.device)
        if x.is_cuda:
            from ._efficientnet_engine import efficientnet_forward
            return efficientnet_forward(self, x, sd.to(x.device))
        return self._forward_torch(x, sd)

    def _apply(self, fn, *a, **kw):
        self._engine = None
        return super()._apply(fn, *a, **kw)


def _efficientnet(width_mult, depth_mult, dropout, pretrained, kw):
    _no_pretrained(pretrained)
    kw.setdefault("dropout", dropout)
    return EfficientNet(width_mult=width_mult, depth_mult=depth_mult, **kw)


def efficientnet_b0(pretrained=False, **kw):
    return _efficientnet(1.0, 1.0, 0.2, pretrained, kw)


def efficientnet_b1(pretrained=False, **kw):
    return _efficientnet(1.0, 1.1, 0.2, pretrained, kw)


def efficientnet_b2(pretrained=False, **kw):
    return _efficientnet(1.1, 1.2, 0.3, pretrained, kw)


def efficientnet_b3(pretrained=False, **kw):
    return _efficientnet(1.2, 1.4, 0.3, pretrained, kw)
