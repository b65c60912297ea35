"""Vision Transformer with the module tree / state-dict names of torchvision.models.vision_transformer (`vit_b_16` and so on:
their checkpoints load strictly), the plain transformer backbone of face-recognition fine-tuning; the FE line is
`model_ = models.vit_b_16(); model_.heads = torch.nn.Linear(768, 512)`.

Restated from the torchvision definition: a patch x patch stride-patch `conv_proj`, a learnt class token in front of the patch
tokens, a learnt position embedding, pre-norm encoder blocks (LayerNorm eps 1e-6 → nn.MultiheadAttention → residual, LayerNorm →
Linear → exact GELU → Linear → residual), a final LayerNorm, and `heads` on the class token.  CPU tensors run these torch layers;
CUDA (HIP) tensors run the gfx950 kernels through models/_vit_engine.ViTEngine (attention over the whole token sequence in
csrc/pfr_mha.hip, everything else on the kernels the Swin engine uses).
"""
import math
from collections import OrderedDict

import torch
import torch.nn as nn

from .resnet import _no_pretrained


class MLPBlock(nn.Sequential):
    """Linear → GELU → Dropout → Linear → Dropout (state-dict keys `0.*` and `3.*`, torchvision's current layout)"""

    def __init__(self, in_dim, mlp_dim, dropout):
        super().__init__(nn.Linear(in_dim, mlp_dim), nn.GELU(), nn.Dropout(dropout), nn.Linear(mlp_dim, in_dim), nn.Dropout(dropout))
        for m in (self[0], self[3]):
            nn.init.xavier_uniform_(m.weight)
            nn.init.normal_(m.bias, std=1e-6)


class EncoderBlock(nn.Module):
    def __init__(self, num_heads, hidden_dim, mlp_dim, dropout, attention_dropout):
        super().__init__()
        self.num_heads = num_heads
        self.ln_1 = nn.LayerNorm(hidden_dim, eps=1e-6)
        self.self_attention = nn.MultiheadAttention(hidden_dim, num_heads, dropout=attention_dropout, batch_first=True)
        self.dropout = nn.Dropout(dropout)
        self.ln_2 = nn.LayerNorm(hidden_dim, eps=1e-6)
        self.mlp = MLPBlock(hidden_dim, mlp_dim, dropout)

    def forward(self, x):
        y = self.ln_1(x)
        y, _ = self.self_attention(y, y, y, need_weights=False)
        x = x + self.dropout(y)
        return x + self.mlp(self.ln_2(x))


class Encoder(nn.Module):
    def __init__(self, seq_length, num_layers, num_heads, hidden_dim, mlp_dim, dropout, attention_dropout):
        super().__init__()
        self.pos_embedding = nn.Parameter(torch.empty(1, seq_length, hidden_dim).normal_(std=0.02))
        self.dropout = nn.Dropout(dropout)
        self.layers = nn.Sequential(OrderedDict((f"encoder_layer_{i}", EncoderBlock(num_heads, hidden_dim, mlp_dim, dropout, attention_dropout))
                                                for i in range(num_layers)))
        self.ln = nn.LayerNorm(hidden_dim, eps=1e-6)

    def forward(self, x):
        return self.ln(self.layers(self.dropout(x + self.pos_embedding)))


class VisionTransformer(nn.Module):
    def __init__(self, image_size=224, patch_size=16, num_layers=12, num_heads=12, hidden_dim=768, mlp_dim=3072, dropout=0.0,
                 attention_dropout=0.0, num_classes=1000, compute_dtype=None):
        super().__init__()
        if image_size % patch_size:
            raise ValueError(f"image_size {image_size} is not a multiple of patch_size {patch_size}")
        if hidden_dim % num_heads:
            raise ValueError(f"hidden_dim {hidden_dim} is not a multiple of num_heads {num_heads}")
        self.image_size, self.patch_size = image_size, patch_size
        self.hidden_dim, self.mlp_dim, self.num_heads = hidden_dim, mlp_dim, num_heads
        self.dropout, self.attention_dropout = float(dropout), float(attention_dropout)
        self.conv_proj = nn.Conv2d(3, hidden_dim, kernel_size=patch_size, stride=patch_size)
        self.seq_length = (image_size // patch_size) ** 2 + 1
        self.class_token = nn.Parameter(torch.zeros(1, 1, hidden_dim))
        self.encoder = Encoder(self.seq_length, num_layers, num_heads, hidden_dim, mlp_dim, dropout, attention_dropout)
        self.heads = nn.Sequential(OrderedDict(head=nn.Linear(hidden_dim, num_classes)))
        fan_in = 3 * patch_size * patch_size
        nn.init.trunc_normal_(self.conv_proj.weight, std=math.sqrt(1 / fan_in))
        nn.init.zeros_(self.conv_proj.bias)
        nn.init.zeros_(self.heads.head.weight)
        nn.init.zeros_(self.heads.head.bias)
        self.compute_dtype = compute_dtype   # HIP compute dtype: torch.bfloat16 / torch.float32 (None → PFR_COMPUTE_DTYPE / bf16)
        self._engine = None

    def _check_input(self, img):
        if img.dim() != 4 or img.shape[1] != 3 or img.shape[2] != self.image_size or img.shape[3] != self.image_size:
            raise ValueError(f"VisionTransformer: expected [N, 3, {self.image_size}, {self.image_size}] (the size pos_embedding was "
                             f"built for; there is no position interpolation), got {tuple(img.shape)}")

    def _forward_torch(self, img):
        x = self.conv_proj(img).flatten(2).transpose(1, 2)                       # [N, S−1, D], row-major patches
        x = torch.cat([self.class_token.expand(x.shape[0], -1, -1), x], dim=1)
        return self.heads(self.encoder(x)[:, 0])

    def hip_engine(self, device=None):
        from ._vit_engine import ViTEngine
        if self._engine is None or not self._engine.matches(self):
            self._engine = ViTEngine(self, device or next(self.parameters()).device, self.compute_dtype)
        return self._engine

    def forward(self, img):
        self._check_input(img)
        if img.is_cuda:
            from ._vit_engine import vit_forward
            if not self.training:      # eval mode: the inference plan, no autograd graph
                with torch.no_grad():
                    return vit_forward(self, img, False)
            return vit_forward(self, img, True)
        return self._forward_torch(img)

    def _apply(self, fn, *a, **kw):
        self._engine = None
        return super()._apply(fn, *a, **kw)


def _vit(defaults, num_classes, pretrained, kw):
    _no_pretrained(pretrained)
    for k, v in defaults.items():
        kw.setdefault(k, v)
    return VisionTransformer(num_classes=num_classes, **kw)


def vit_b_16(num_classes=1000, pretrained=False, **kw):
    return _vit(dict(patch_size=16, num_layers=12, num_heads=12, hidden_dim=768, mlp_dim=3072), num_classes, pretrained, kw)


def vit_b_32(num_classes=1000, pretrained=False, **kw):
    return _vit(dict(patch_size=32, num_layers=12, num_heads=12, hidden_dim=768, mlp_dim=3072), num_classes, pretrained, kw)


def vit_l_16(num_classes=1000, pretrained=False, **kw):
    return _vit(dict(patch_size=16, num_layers=24, num_heads=16, hidden_dim=1024, mlp_dim=4096), num_classes, pretrained, kw)


def vit_s_16(num_classes=1000, pretrained=False, **kw):
    """DeiT-S geometry: 384 wide, 6 heads (head_dim 64), MLP 1536, 12 layers"""
    return _vit(dict(patch_size=16, num_layers=12, num_heads=6, hidden_dim=384, mlp_dim=1536), num_classes, pretrained, kw)


def vit_t_16(num_classes=1000, pretrained=False, **kw):
    """DeiT-Ti geometry: 192 wide, 3 heads (head_dim 64), MLP 768, 12 layers"""
    return _vit(dict(patch_size=16, num_layers=12, num_heads=3, hidden_dim=192, mlp_dim=768), num_classes, pretrained, kw)
