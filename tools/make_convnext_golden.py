"""Writes tests/golden/convnext_hf.npz: outputs of an INDEPENDENT ConvNeXt implementation (Hugging Face `transformers`
ConvNextModel) that tests/test_convnext_host.py pins this project's models/convnext.py to.

A small net (hidden_sizes 32-64-96-128, depths 1-1-2-1, layer_norm_eps 1e-6 — HF's final LayerNorm defaults to 1e-12 —,
drop_path_rate 0) is filled from numpy.random.default_rng(seed) in sorted key order by fill_param() below (the test carries
the same function), fed a seeded [2,3,64,64] input in fp64, and the fixture keeps numbers and key names only: the seed, the
key list with shapes, the pooled output [2,128] and, for every parameter's gradient g of pooled.square().sum() in fp64:
its sum, sum |g|, and its projection sum g*r on a seeded standard-normal r (drawn after the input, in the same key order).
The plain sum is mathematically zero for the seven parameters that feed a LayerNorm directly (stem conv, depthwise biases):
the projection and sum |g| are the quantities that pin those.  No weights are stored.   python tools/make_convnext_golden.py"""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240


def fill_param(rng, key, shape):
    """layer scale and LayerNorm weights uniform in [0.5, 1.5], biases N(0, 0.1²), conv / Linear weights N(0, 1/fan_in)"""
    if key.endswith("layer_scale_parameter") or (key.endswith("weight") and len(shape) == 1):
        return rng.uniform(0.5, 1.5, size=shape)
    if key.endswith("bias"):
        return rng.standard_normal(shape) * 0.1
    fan_in = int(np.prod(shape[1:]))
    return rng.standard_normal(shape) / np.sqrt(fan_in)


def main():
    from transformers import ConvNextConfig, ConvNextModel
    cfg = ConvNextConfig(hidden_sizes=[32, 64, 96, 128], depths=[1, 1, 2, 1], layer_norm_eps=1e-6, drop_path_rate=0.0)
    m = ConvNextModel(cfg).double().eval()
    rng = np.random.default_rng(SEED)
    params = dict(m.named_parameters())
    keys = sorted(params)
    with torch.no_grad():
        for k in keys:
            params[k].copy_(torch.from_numpy(fill_param(rng, k, tuple(params[k].shape))))
    x = torch.from_numpy(rng.standard_normal((2, 3, 64, 64)))
    pooled = m(pixel_values=x).pooler_output
    pooled.square().sum().backward()
    grads = [params[k].grad for k in keys]
    proj = [(g * torch.from_numpy(rng.standard_normal(tuple(g.shape)))).sum().item() for g in grads]
    out = os.path.join(ROOT, "tests", "golden", "convnext_hf.npz")
    np.savez(out, seed=np.int64(SEED), keys=np.array(keys), shapes=np.array([",".join(map(str, params[k].shape)) for k in keys]),
             pooled=pooled.detach().numpy(), grad_sums=np.array([g.sum().item() for g in grads], dtype=np.float64),
             grad_abs_sums=np.array([g.abs().sum().item() for g in grads], dtype=np.float64),
             grad_proj=np.array(proj, dtype=np.float64))
    print(f"{out}: {len(keys)} parameters, pooled {tuple(pooled.shape)}, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
