"""IResNet ("improved ResNet") with the module tree / state-dict names of the public insightface arcface_torch backbone — the
network the ArcFace, AdaFace, CurricularFace and Partial FC margins of losses/ were published with.

Restated from that definition: 112x112 aligned crops, a 3x3 stride-1 stem without max-pool (Conv → BatchNorm → PReLU), four
layers of pre-activation IBasicBlocks (BN → conv3x3 → BN → PReLU → conv3x3 stride s → BN, plus the identity or a 1x1 strided
conv → BN shortcut, no activation after the add), every layer's first block with stride 2, and the embedding neck BatchNorm2d →
flatten (NCHW order) → Dropout → Linear → BatchNorm1d whose weight is fixed at 1.  `input_size` is the one argument the public
definition does not have (it fixes 112, i.e. fc_scale = 7 * 7): the Linear's fan-in follows from it.  CPU tensors run these torch
layers; CUDA (HIP) tensors run the gfx950 kernels through models/_iresnet_engine.IResNetEngine (the PReLU forms of the BatchNorm
kernels in csrc/pfr_prelu.hip, everything else on the kernels the other BatchNorm engines use).
"""
import torch
import torch.nn as nn

from .resnet import _no_pretrained


def _conv3x3(inp, oup, stride=1):
    return nn.Conv2d(inp, oup, 3, stride, 1, bias=False)


class IBasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(inplanes, eps=1e-05)
        self.conv1 = _conv3x3(inplanes, planes)
        self.bn2 = nn.BatchNorm2d(planes, eps=1e-05)
        self.prelu = nn.PReLU(planes)
        self.conv2 = _conv3x3(planes, planes, stride)
        self.bn3 = nn.BatchNorm2d(planes, eps=1e-05)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = self.bn3(self.conv2(self.prelu(self.bn2(self.conv1(self.bn1(x))))))
        return out + (x if self.downsample is None else self.downsample(x))


def _out_size(s):
    """spatial size after the four stride-2 layers (3x3, padding 1: (s - 1) // 2 + 1 each)"""
    for _ in range(4):
        s = (s - 1) // 2 + 1
    return s


class IResNet(nn.Module):
    def __init__(self, block, layers, dropout=0, num_features=512, zero_init_residual=False, input_size=112, compute_dtype=None):
        super().__init__()
        self.inplanes = 64
        self.input_size = int(input_size)
        s = _out_size(self.input_size)
        self.fc_scale = s * s
        self.conv1 = _conv3x3(3, self.inplanes)
        self.bn1 = nn.BatchNorm2d(self.inplanes, eps=1e-05)
        self.prelu = nn.PReLU(self.inplanes)
        self.layer1 = self._make_layer(block, 64, layers[0], stride=2)
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.bn2 = nn.BatchNorm2d(512 * block.expansion, eps=1e-05)
        self.dropout = nn.Dropout(p=dropout, inplace=True)
        self.fc = nn.Linear(512 * block.expansion * self.fc_scale, num_features)
        self.features = nn.BatchNorm1d(num_features, eps=1e-05)
        nn.init.constant_(self.features.weight, 1.0)
        self.features.weight.requires_grad = False
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0, 0.1)
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, IBasicBlock):
                    nn.init.constant_(m.bn3.weight, 0)      # the block's last BatchNorm: every block starts as its shortcut
        self.compute_dtype = compute_dtype   # HIP compute dtype: torch.bfloat16 / torch.float32 (None → PFR_COMPUTE_DTYPE / bf16)
        self._engine = None

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * block.expansion, 1, stride, bias=False),
                                       nn.BatchNorm2d(planes * block.expansion, eps=1e-05))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes))
        return nn.Sequential(*layers)

    def _forward_torch(self, x):
        x = self.prelu(self.bn1(self.conv1(x)))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = self.dropout(torch.flatten(self.bn2(x), 1))
        return self.features(self.fc(x))

    def hip_engine(self, device=None):
        from ._iresnet_engine import IResNetEngine
        if self._engine is None or not self._engine.matches(self):
            self._engine = IResNetEngine(self, device or next(self.parameters()).device, self.compute_dtype)
        return self._engine

    def forward(self, x):
        if x.is_cuda:
            from ._iresnet_engine import iresnet_forward
            return iresnet_forward(self, x)
        return self._forward_torch(x)

    def _apply(self, fn, *a, **kw):
        self._engine = None
        return super()._apply(fn, *a, **kw)


def _iresnet(layers, pretrained, kw):
    _no_pretrained(pretrained)
    return IResNet(IBasicBlock, layers, **kw)


def iresnet18(pretrained=False, **kw):
    return _iresnet([2, 2, 2, 2], pretrained, kw)


def iresnet34(pretrained=False, **kw):
    return _iresnet([3, 4, 6, 3], pretrained, kw)


def iresnet50(pretrained=False, **kw):
    return _iresnet([3, 4, 14, 3], pretrained, kw)


def iresnet100(pretrained=False, **kw):
    return _iresnet([3, 13, 30, 3], pretrained, kw)


def iresnet200(pretrained=False, **kw):
    return _iresnet([6, 26, 60, 6], pretrained, kw)
