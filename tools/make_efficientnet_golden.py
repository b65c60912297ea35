"""Writes tests/golden/efficientnet_b2_hf.npz: the output of an INDEPENDENT EfficientNet-B2 implementation (Hugging Face `transformers`
EfficientNetModel) that tests/test_efficientnet_host.py pins this project's models/efficientnet.py to.

B2's config (width_coefficient 1.1, depth_coefficient 1.2, hidden_dim 1408, depthwise_padding [], batch_norm_eps 1e-5; everything else
the B0 table both implementations start from) is filled from numpy.random.default_rng(seed) in state-dict order by fill_entry() below
(the test carries the same function) — running statistics included, since the comparison runs in EVAL mode and fp64.  The two
state dicts list the same tensors in the same order (stem, per block expand / depthwise / squeeze-excite / project, top conv), so the
test maps Hugging Face keys to torchvision keys by position and checks every shape.

Padding: Hugging Face pads every stride-2 convolution on the bottom / right only (ZeroPad2d + 'valid'), torchvision symmetrically.  At
even plane sizes the two are mirror images: conv2d(x, w, stride=2, padding=k//2) equals the Hugging Face form applied to x.flip(2, 3)
with w.flip(2, 3), flipped back; stride-1 'same' convolutions, 1x1 convolutions, squeeze-excite and the global mean are flip-invariant.
So this tool feeds the FLIPPED input and the test loads every k x k kernel flipped; the pooled outputs then agree.  The input is
[2,3,64,64]: every plane entering a stride-2 layer (64, 32, 16, 8, 4) is even.

The fixture keeps numbers and key names only: the seed, the key list with shapes, the (unflipped) input and the pooled output
[2,1408].  No weights are stored.   python tools/make_efficientnet_golden.py"""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20242


def fill_entry(rng, key, shape):
    """BatchNorm weights and running variances uniform in [0.5, 1.5], biases and running means N(0, 0.1²), conv weights N(0, 2/fan_in)"""
    if key.endswith("running_var") or (key.endswith("weight") and len(shape) == 1):
        return rng.uniform(0.5, 1.5, size=shape)
    if key.endswith("bias") or key.endswith("running_mean"):
        return rng.standard_normal(shape) * 0.1
    fan_in = int(np.prod(shape[1:]))
    return rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)


def main():
    from transformers import EfficientNetConfig, EfficientNetModel
    cfg = EfficientNetConfig(width_coefficient=1.1, depth_coefficient=1.2, hidden_dim=1408, depthwise_padding=[], batch_norm_eps=1e-5,
                             image_size=64)
    m = EfficientNetModel(cfg).double().eval()
    rng = np.random.default_rng(SEED)
    sd = m.state_dict()
    keys = [k for k in sd if not k.endswith("num_batches_tracked")]
    with torch.no_grad():
        for k in keys:
            sd[k].copy_(torch.from_numpy(fill_entry(rng, k, tuple(sd[k].shape))))
    x = rng.standard_normal((2, 3, 64, 64))
    with torch.no_grad():
        pooled = m(pixel_values=torch.from_numpy(x).flip(2, 3)).pooler_output
    out = os.path.join(ROOT, "tests", "golden", "efficientnet_b2_hf.npz")
    np.savez(out, seed=np.int64(SEED), keys=np.array(keys), shapes=np.array([",".join(map(str, sd[k].shape)) for k in keys]),
             x=x, pooled=pooled.numpy())
    print(f"{out}: {len(keys)} entries, pooled {tuple(pooled.shape)}, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
