"""ConvNeXt with the module tree / state-dict names of torchvision.models.convnext (the alternative backbone of
the reference's configs/dog_fe/masked_head_dog.py:105-106: `convnext_tiny(pretrained=True)` with `classifier[2] = Linear(768, 512)`).

Restated from the torchvision definition: 4x4 stride-4 patchify stem + LayerNorm2d, four stages of CNBlocks (depthwise 7x7 conv →
LayerNorm → Linear C→4C → GELU → Linear 4C→C, layer scale, "row" stochastic depth, residual) with LayerNorm2d + 2x2 stride-2 conv
between them, avgpool → LayerNorm2d → Flatten → Linear.  CPU tensors run these torch layers; CUDA (HIP) tensors run the gfx950
kernels through models/_convnext_engine.ConvNeXtEngine (depthwise conv and layer scale in csrc/pfr_dwconv.hip, everything else on
the kernels the Swin engine uses).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .resnet import _no_pretrained


class LayerNorm2d(nn.LayerNorm):
    """LayerNorm over the channels of an NCHW tensor"""

    def forward(self, x):
        x = x.permute(0, 2, 3, 1)
        x = F.layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps)
        return x.permute(0, 3, 1, 2)


class Permute(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.dims = dims

    def forward(self, x):
        return x.permute(*self.dims)


class CNBlock(nn.Module):
    def __init__(self, dim, layer_scale, sd_prob):
        super().__init__()
        self.block = nn.Sequential(
            nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim, bias=True),
            Permute([0, 2, 3, 1]),
            nn.LayerNorm(dim, eps=1e-6),
            nn.Linear(dim, 4 * dim, bias=True),
            nn.GELU(),
            nn.Linear(4 * dim, dim, bias=True),
            Permute([0, 3, 1, 2]),
        )
        self.layer_scale = nn.Parameter(torch.ones(dim, 1, 1) * layer_scale)
        self.sd_prob = sd_prob   # stochastic depth, mode "row": a whole sample's branch is dropped with this probability

    def forward(self, x, sd=None):
        """sd: this block's row of ConvNeXt._draw_sd (fp32 [N]: 0 or 1/(1-p)), None = keep every sample unscaled"""
        r = self.layer_scale * self.block(x)
        if sd is not None:
            r = r * sd.view(-1, 1, 1, 1).to(r.dtype)
        return x + r


class ConvNeXt(nn.Module):
    def __init__(self, depths=(3, 3, 9, 3), dims=(96, 192, 384, 768), stochastic_depth_prob=0.0, layer_scale=1e-6,
                 num_classes=1000, block_setting=None, compute_dtype=None):
        super().__init__()
        if block_setting is not None:
            # torchvision's list of CNBlockConfig(input_channels, out_channels | None, num_layers), or plain tuples of the same three
            dims = tuple(b.input_channels if hasattr(b, "input_channels") else b[0] for b in block_setting)
            depths = tuple(b.num_layers if hasattr(b, "num_layers") else b[2] for b in block_setting)
        if len(dims) != len(depths) or not dims:
            raise ValueError("depths and dims must have the same, non-zero length")
        self.depths, self.dims = tuple(depths), tuple(dims)
        self.stochastic_depth_prob = float(stochastic_depth_prob)
        n_blocks = sum(depths)
        self.sd_probs = [self.stochastic_depth_prob * i / (n_blocks - 1.0) if n_blocks > 1 else 0.0 for i in range(n_blocks)]
        layers = [nn.Sequential(nn.Conv2d(3, dims[0], kernel_size=4, stride=4, padding=0, bias=True), LayerNorm2d(dims[0], eps=1e-6))]
        bid = 0
        for si, (d, n) in enumerate(zip(dims, depths)):
            layers.append(nn.Sequential(*[CNBlock(d, layer_scale, self.sd_probs[bid + j]) for j in range(n)]))
            bid += n
            if si + 1 < len(dims):
                layers.append(nn.Sequential(LayerNorm2d(d, eps=1e-6), nn.Conv2d(d, dims[si + 1], kernel_size=2, stride=2)))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        # num_classes = 0: the pooled, normalised features themselves
        self.classifier = nn.Sequential(LayerNorm2d(dims[-1], eps=1e-6), nn.Flatten(1),
                                        nn.Linear(dims[-1], num_classes) if num_classes > 0 else nn.Identity())
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
        self._sd_p = {}   # device -> the block probabilities as a tensor (built once: no host-to-device copy per forward)
        self.compute_dtype = compute_dtype   # HIP compute dtype: torch.bfloat16 / torch.float32 (None → PFR_COMPUTE_DTYPE / bf16)
        self._engine = None

    def blocks(self):
        """the CNBlocks in forward order"""
        return [b for st in self.features if isinstance(st[0], CNBlock) for b in st]

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

    def _forward_torch(self, img, sd):
        x = img
        bid = 0
        for st in self.features:
            if isinstance(st[0], CNBlock):
                for blk in st:
                    x = blk(x, sd[bid])
                    bid += 1
            else:
                x = st(x)
        return self.classifier(self.avgpool(x))

    def hip_engine(self, device=None):
        from ._convnext_engine import ConvNeXtEngine
        if self._engine is None or not self._engine.matches(self):
            self._engine = ConvNeXtEngine(self, device or next(self.parameters()).device, self.compute_dtype)
        return self._engine

    def forward(self, img):
        sd = self._draw_sd(img.shape[0], img.device)
        if img.is_cuda:
            from ._convnext_engine import convnext_forward
            return convnext_forward(self, img, sd)
        return self._forward_torch(img, sd)

    def _apply(self, fn, *a, **kw):
        self._engine = None
        return super()._apply(fn, *a, **kw)


def convnext_tiny(num_classes=1000, pretrained=False, **kw):
    _no_pretrained(pretrained)
    kw.setdefault("stochastic_depth_prob", 0.1)
    kw.setdefault("depths", (3, 3, 9, 3))
    kw.setdefault("dims", (96, 192, 384, 768))
    return ConvNeXt(num_classes=num_classes, **kw)


def convnext_small(num_classes=1000, pretrained=False, **kw):
    _no_pretrained(pretrained)
    kw.setdefault("stochastic_depth_prob", 0.4)
    kw.setdefault("depths", (3, 3, 27, 3))
    kw.setdefault("dims", (96, 192, 384, 768))
    return ConvNeXt(num_classes=num_classes, **kw)
