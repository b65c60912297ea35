"""Writes tests/golden/mobilenet_v2_hf.npz: the output of an INDEPENDENT MobileNetV2 implementation (Hugging Face `transformers`
MobileNetV2Model) that tests/test_mobilenet_host.py pins this project's models/mobilenet.py to.

The full-width net (tf_padding False: symmetric padding 1 as torchvision; layer_norm_eps 1e-5 = the BatchNorm eps; depth_multiplier 1,
finegrained_output and first_layer_is_expansion True: torchvision's channel table and its t = 1 first block) is filled from
numpy.random.default_rng(seed) in sorted state-dict key order by fill_entry() below (the test carries the same function) — running
statistics included, since the comparison runs in EVAL mode (the Hugging Face BatchNorm momentum differs and plays no part there) — and
fed a seeded [2,3,64,64] input in fp64.  The fixture keeps numbers and key names only: the seed, the key list with shapes, the
input and the pooled output [2,1280].  No weights are stored.   python tools/make_mobilenet_golden.py"""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20241


def fill_entry(rng, key, shape):
    """BatchNorm weights and running variances uniform in [0.5, 1.5], biases and running means N(0, 0.1²), conv weights N(0, 2/fan_in)"""
    if key.endswith("running_var") or (key.endswith("weight") and len(shape) == 1):
        return rng.uniform(0.5, 1.5, size=shape)
    if key.endswith("bias") or key.endswith("running_mean"):
        return rng.standard_normal(shape) * 0.1
    fan_in = int(np.prod(shape[1:]))
    return rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)


def main():
    from transformers import MobileNetV2Config, MobileNetV2Model
    cfg = MobileNetV2Config(tf_padding=False, layer_norm_eps=1e-5, depth_multiplier=1.0, finegrained_output=True,
                            first_layer_is_expansion=True)
    m = MobileNetV2Model(cfg).double().eval()
    rng = np.random.default_rng(SEED)
    sd = m.state_dict()
    keys = sorted(k for k in sd if not k.endswith("num_batches_tracked"))
    with torch.no_grad():
        for k in keys:
            sd[k].copy_(torch.from_numpy(fill_entry(rng, k, tuple(sd[k].shape))))
    x = rng.standard_normal((2, 3, 64, 64))
    with torch.no_grad():
        pooled = m(pixel_values=torch.from_numpy(x)).pooler_output
    out = os.path.join(ROOT, "tests", "golden", "mobilenet_v2_hf.npz")
    np.savez(out, seed=np.int64(SEED), keys=np.array(keys), shapes=np.array([",".join(map(str, sd[k].shape)) for k in keys]),
             x=x, pooled=pooled.numpy())
    print(f"{out}: {len(keys)} entries, pooled {tuple(pooled.shape)}, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
