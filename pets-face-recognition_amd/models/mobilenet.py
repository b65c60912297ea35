"""MobileNetV2 with the module tree / state-dict names of torchvision.models.mobilenetv2 (the first alternative backbone of the
reference's feature-extractor configs, configs/dog_fe/fe_dogs_config.py:104-105: `mobilenet_v2(pretrained=True)` with
`classifier = Sequential(Linear(last_channel, 512))`).

Restated from the torchvision definition: 3x3 stride-2 stem (Conv → BatchNorm → ReLU6), inverted-residual blocks (1x1 expand →
BN → ReLU6 unless t = 1, depthwise 3x3 stride s → BN → ReLU6, 1x1 project → BN, residual when stride 1 and inp == oup), a last
1x1 conv → BN → ReLU6 to `last_channel`, avgpool → Dropout → Linear.  CPU tensors run these torch layers; CUDA (HIP) tensors run
the gfx950 kernels through models/_mobilenet_engine.MobileNetV2Engine (depthwise conv in csrc/pfr_dwconv3.hip, the ReLU6 forms of
the BatchNorm kernels, everything else on the kernels the ResNet engine uses).
"""
import torch
import torch.nn as nn

from .resnet import _no_pretrained


def _make_divisible(v, divisor=8, min_value=None):
    """torchvision.models._utils._make_divisible: the nearest multiple of `divisor`, never more than 10 % below v"""
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def _conv_bn_relu6(inp, oup, kernel_size=3, stride=1, groups=1):
    """torchvision's Conv2dNormActivation(norm_layer=BatchNorm2d, activation_layer=ReLU6): keys 0.weight, 1.*"""
    return nn.Sequential(nn.Conv2d(inp, oup, kernel_size, stride, (kernel_size - 1) // 2, groups=groups, bias=False),
                         nn.BatchNorm2d(oup), nn.ReLU6(inplace=True))


class InvertedResidual(nn.Module):
    def __init__(self, inp, oup, stride, expand_ratio):
        super().__init__()
        if stride not in (1, 2):
            raise ValueError(f"stride should be 1 or 2 instead of {stride}")
        self.stride = stride
        hidden = int(round(inp * expand_ratio))
        self.use_res_connect = stride == 1 and inp == oup
        layers = []
        if expand_ratio != 1:
            layers.append(_conv_bn_relu6(inp, hidden, kernel_size=1))
        layers += [_conv_bn_relu6(hidden, hidden, stride=stride, groups=hidden),
                   nn.Conv2d(hidden, oup, 1, 1, 0, bias=False), nn.BatchNorm2d(oup)]
        self.conv = nn.Sequential(*layers)
        self.out_channels = oup

    def forward(self, x):
        return x + self.conv(x) if self.use_res_connect else self.conv(x)


class MobileNetV2(nn.Module):
    def __init__(self, num_classes=1000, width_mult=1.0, inverted_residual_setting=None, round_nearest=8, dropout=0.2,
                 compute_dtype=None):
        super().__init__()
        input_channel, last_channel = 32, 1280
        if inverted_residual_setting is None:
            inverted_residual_setting = [[1, 16, 1, 1], [6, 24, 2, 2], [6, 32, 3, 2], [6, 64, 4, 2], [6, 96, 3, 1], [6, 160, 3, 2],
                                         [6, 320, 1, 1]]     # t, c, n, s
        if len(inverted_residual_setting) == 0 or len(inverted_residual_setting[0]) != 4:
            raise ValueError(f"inverted_residual_setting should be non-empty or a 4-element list, got {inverted_residual_setting}")
        input_channel = _make_divisible(input_channel * width_mult, round_nearest)
        self.last_channel = _make_divisible(last_channel * max(1.0, width_mult), round_nearest)
        features = [_conv_bn_relu6(3, input_channel, stride=2)]
        for t, c, n, s in inverted_residual_setting:
            output_channel = _make_divisible(c * width_mult, round_nearest)
            for i in range(n):
                features.append(InvertedResidual(input_channel, output_channel, s if i == 0 else 1, expand_ratio=t))
                input_channel = output_channel
        features.append(_conv_bn_relu6(input_channel, self.last_channel, kernel_size=1))
        self.features = nn.Sequential(*features)
        self.classifier = nn.Sequential(nn.Dropout(p=dropout), nn.Linear(self.last_channel, num_classes))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.zeros_(m.bias)
        self.compute_dtype = compute_dtype   # HIP compute dtype: torch.bfloat16 / torch.float32 (None → PFR_COMPUTE_DTYPE / bf16)
        self._engine = None

    def _forward_torch(self, x):
        x = self.features(x)
        x = nn.functional.adaptive_avg_pool2d(x, (1, 1))
        return self.classifier(torch.flatten(x, 1))

    def hip_engine(self, device=None):
        from ._mobilenet_engine import MobileNetV2Engine
        if self._engine is None or not self._engine.matches(self):
            self._engine = MobileNetV2Engine(self, device or next(self.parameters()).device, self.compute_dtype)
        return self._engine

    def forward(self, x):
        if x.is_cuda:
            from ._mobilenet_engine import mobilenet_forward
            return mobilenet_forward(self, x)
        return self._forward_torch(x)

    def _apply(self, fn, *a, **kw):
        self._engine = None
        return super()._apply(fn, *a, **kw)


def mobilenet_v2(pretrained=False, **kw):
    _no_pretrained(pretrained)
    return MobileNetV2(**kw)
