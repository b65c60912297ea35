"""ConvNeXt on the host: torchvision's state-dict layout, the CPU module against an independent implementation (Hugging Face
ConvNextModel, fixture written by tools/make_convnext_golden.py), the stochastic-depth draw, and the argument checks of the new
C-ABI entries (no device work)."""
import ctypes
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _torchvision_keys(num_classes=512, depths=(3, 3, 9, 3), dims=(96, 192, 384, 768)):
    """torchvision.models.convnext_tiny().state_dict() keys → shapes, written out"""
    k = {"features.0.0.weight": (dims[0], 3, 4, 4), "features.0.0.bias": (dims[0],),
         "features.0.1.weight": (dims[0],), "features.0.1.bias": (dims[0],)}
    for s, (n, C) in enumerate(zip(depths, dims)):
        for j in range(n):
            p = f"features.{2 * s + 1}.{j}."
            k[p + "layer_scale"] = (C, 1, 1)
            k[p + "block.0.weight"] = (C, 1, 7, 7)
            k[p + "block.0.bias"] = (C,)
            k[p + "block.2.weight"] = (C,)
            k[p + "block.2.bias"] = (C,)
            k[p + "block.3.weight"] = (4 * C, C)
            k[p + "block.3.bias"] = (4 * C,)
            k[p + "block.5.weight"] = (C, 4 * C)
            k[p + "block.5.bias"] = (C,)
        if s + 1 < len(dims):
            p = f"features.{2 * s + 2}."
            k[p + "0.weight"] = (C,)
            k[p + "0.bias"] = (C,)
            k[p + "1.weight"] = (dims[s + 1], C, 2, 2)
            k[p + "1.bias"] = (dims[s + 1],)
    k["classifier.0.weight"] = (dims[-1],)
    k["classifier.0.bias"] = (dims[-1],)
    k["classifier.2.weight"] = (num_classes, dims[-1])
    k["classifier.2.bias"] = (num_classes,)
    return k


def test_state_dict_keys_and_shapes_are_torchvisions():
    import pets_face_recognition_amd.models as M
    m = M.convnext_tiny(num_classes=512)
    want = _torchvision_keys()
    assert len(want) == 4 + 18 * 9 + 3 * 4 + 4
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    assert len(m.blocks()) == 18
    # a checkpoint with those keys loads strictly; so does the reference config's head swap
    g = torch.Generator().manual_seed(0)
    sd = {k: torch.randn(s, generator=g) for k, s in want.items()}
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.features[1][0].block[0].weight, sd["features.1.0.block.0.weight"])
    m2 = M.convnext_tiny(pretrained=False)
    m2.classifier[2] = torch.nn.Linear(768, 512)
    m2.load_state_dict(sd, strict=True)
    # details of the definition
    assert m.features[0][1].eps == 1e-6 and m.classifier[0].eps == 1e-6 and m.features[1][0].block[2].eps == 1e-6
    fresh = M.convnext_tiny(num_classes=8)
    assert torch.all(fresh.features[1][0].layer_scale == 1e-6)
    assert abs(fresh.features[1][0].block[3].weight.std().item() - 0.02) < 1e-3     # trunc-normal(0.02); 36864 weights
    assert torch.all(fresh.features[1][0].block[3].bias == 0)
    assert len(M.convnext_small(num_classes=8).blocks()) == 36


def test_pretrained_flag_warns():
    import pets_face_recognition_amd.models as M
    with pytest.warns(UserWarning, match="pretrained=True ignored"):
        M.convnext_tiny(pretrained=True, depths=(1, 1), dims=(8, 16), num_classes=4)


def _fill_param(rng, key, shape):
    """tools/make_convnext_golden.py:fill_param"""
    if key.endswith("layer_scale_parameter") or (key.endswith("weight") and len(shape) == 1):
        return rng.uniform(0.5, 1.5, size=shape)
    if key.endswith("bias"):
        return rng.standard_normal(shape) * 0.1
    fan_in = int(np.prod(shape[1:]))
    return rng.standard_normal(shape) / np.sqrt(fan_in)


def _hf_to_ours(key):
    """Hugging Face ConvNextModel parameter name → torchvision name (written out)"""
    t = key.split(".")
    if t[0] == "embeddings":
        return {"patch_embeddings": "features.0.0.", "layernorm": "features.0.1."}[t[1]] + t[2]
    if t[0] == "layernorm":
        return "classifier.0." + t[1]
    assert t[0] == "encoder" and t[1] == "stages"
    s = int(t[2])
    if t[3] == "downsampling_layer":
        return f"features.{2 * s}.{t[4]}.{t[5]}"
    assert t[3] == "layers"
    pre = f"features.{2 * s + 1}.{t[4]}."
    if t[5] == "layer_scale_parameter":
        return pre + "layer_scale"
    return pre + {"dwconv": "block.0.", "layernorm": "block.2.", "pwconv1": "block.3.", "pwconv2": "block.5."}[t[5]] + t[6]


def test_cpu_module_matches_huggingface_convnext():
    """Pooled output within 1e-5 relative; per parameter, the gradient of pooled.square().sum() (both sides fp64): its projection
    on a seeded random tensor and sum |g| within 1e-4 relative — non-degenerate for every parameter — and its plain sum within 1e-4
    relative wherever that sum is a number and not rounding residue.  A shift of a LayerNorm's input changes nothing, so the sums
    for the stem conv and the depthwise biases are mathematically zero: what fp64 leaves there (1e-15 .. 1e-13 against
    sum |g| of 1 .. 1e3) depends on the reduction order, i.e. on the thread count.  An fp64 sum of n <= 5e4 terms is off by at most
    n * 2^-53 * sum |g| ~ 5e-12 * sum |g|; a relative bound of 1e-4 on it means something only above 1e4 times that, so below
    1e-7 * sum |g| the assertion is that the sum IS zero to that level on both sides."""
    import pets_face_recognition_amd.models as M
    G = np.load(os.path.join(GOLD, "convnext_hf.npz"))
    keys = [str(k) for k in G["keys"]]
    shapes = [tuple(int(v) for v in str(s).split(",")) for s in G["shapes"]]
    m = M.ConvNeXt(depths=(1, 1, 2, 1), dims=(32, 64, 96, 128), num_classes=0, stochastic_depth_prob=0.0).double().eval()
    ours = dict(m.named_parameters())
    rng = np.random.default_rng(int(G["seed"]))
    names = []
    with torch.no_grad():
        for k, s in zip(keys, shapes):
            n = _hf_to_ours(k)
            names.append(n)
            v = torch.from_numpy(_fill_param(rng, k, s))
            ours[n].copy_(v.view(ours[n].shape))
    assert sorted(names) == sorted(ours), "every parameter of the module is filled from the fixture's key list"
    x = torch.from_numpy(rng.standard_normal((2, 3, 64, 64)))
    pooled = m(x)
    assert tuple(pooled.shape) == (2, 128)
    want = torch.from_numpy(G["pooled"])
    e = ((pooled.detach() - want).norm() / want.norm()).item()
    print(f"pooled rel err {e:.3e}")
    assert e < 1e-5
    pooled.square().sum().backward()
    degenerate = []
    for n, s, gs, ga, gp in zip(names, shapes, G["grad_sums"], G["grad_abs_sums"], G["grad_proj"]):
        g = ours[n].grad
        r = torch.from_numpy(rng.standard_normal(s)).view(g.shape)
        assert ga > 0 and abs(gp) > 1e-6 * ga, (n, ga, gp)                  # the recorded quantities are not degenerate
        assert abs((g * r).sum().item() - gp) <= 1e-4 * abs(gp), (n, (g * r).sum().item(), gp)
        assert abs(g.abs().sum().item() - ga) <= 1e-4 * ga, (n, g.abs().sum().item(), ga)
        got = g.sum().item()
        if abs(gs) > 1e-7 * ga:
            assert abs(got - gs) <= 1e-4 * abs(gs), (n, got, gs)
        else:
            degenerate.append(n)
            assert abs(got) <= 1e-7 * ga, (n, got, ga)
    # exactly the parameters whose output goes straight into a LayerNorm
    assert sorted(degenerate) == sorted(["features.0.0.weight", "features.0.0.bias"] + [n for n in names if n.endswith("block.0.bias")])


def test_draw_sd_and_training_forward():
    import pets_face_recognition_amd.models as M
    torch.manual_seed(3)
    m = M.ConvNeXt(depths=(1, 1, 2, 1), dims=(8, 16, 24, 32), num_classes=6, stochastic_depth_prob=0.4)
    n = 5
    assert m.sd_probs == pytest.approx([0.4 * i / (n - 1) for i in range(n)])
    assert [b.sd_prob for b in m.blocks()] == m.sd_probs
    m.train()
    d = m._draw_sd(4000, "cpu")
    assert d.dtype == torch.float32 and tuple(d.shape) == (n, 4000)
    for i, p in enumerate(m.sd_probs):
        vals = d[i].unique().tolist()
        assert all(v == 0.0 or abs(v - 1.0 / (1.0 - p)) < 1e-6 for v in vals), (i, vals)
        assert abs((d[i] == 0).float().mean().item() - p) < 0.05      # 4000 draws: sigma <= 0.008
    assert torch.all(d[0] == 1)
    m.eval()
    assert torch.all(m._draw_sd(7, "cpu") == 1)
    assert torch.all(M.ConvNeXt(depths=(1, 1), dims=(8, 16), num_classes=4).train()._draw_sd(3, "cpu") == 1)   # p = 0

    # fixed draw: the training forward is x + sd·γ·branch(x) block by block
    m.train()
    with torch.no_grad():
        for b in m.blocks():
            b.layer_scale.uniform_(0.5, 1.5)
    fixed = torch.ones(n, 3)
    fixed[2, 1] = 0.0
    fixed[4, 0] = 0.0
    fixed[3, 2] = 1.0 / (1.0 - m.sd_probs[3])
    calls = []
    m._draw_sd = lambda N, device: (calls.append(N), fixed)[1]
    x = torch.randn(3, 3, 64, 64)
    out = m(x)
    assert calls == [3]
    h = x
    bid = 0
    for st in m.features:
        if isinstance(st[0], M.convnext.CNBlock):
            for blk in st:
                h = h + fixed[bid].view(-1, 1, 1, 1) * blk.layer_scale * blk.block(h)
                bid += 1
        else:
            h = st(h)
    want = m.classifier(m.avgpool(h))
    assert torch.allclose(out, want, rtol=1e-5, atol=1e-6)
    # a dropped sample passes its block unchanged
    blk = m.features[1][0]
    t = torch.randn(2, 8, 16, 16)
    assert torch.equal(blk(t, torch.tensor([0.0, 1.0]))[0], t[0])


def test_new_entries_report_argument_errors():
    """K != 7, null and host pointers: an error code (PfrError through the binding), never a crash"""
    from pets_face_recognition_amd._hip import lib, PfrError
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    with pytest.raises(PfrError, match="K = 7"):
        lib.pfr_dwconv2d_fwd(p, p, 0, p, 0, 1, 4, 4, 8, 3, 0, 0)
    with pytest.raises(PfrError, match="K = 7"):
        lib.pfr_dwconv2d_wgrad(p, p, p, p, 0, 0, 1, 4, 4, 8, 5, 0, 0)
    assert lib.pfr_dwconv2d_wgrad_parts(0, 1, 4, 4, 8, 3) == 0
    assert lib.pfr_dwconv2d_wgrad_parts(1, 128, 56, 56, 96, 7) >= 1
    assert lib.pfr_layer_scale_bwd_parts(2, 49, 768) >= 1
    with pytest.raises(PfrError, match="null pointer"):
        lib.pfr_dwconv2d_fwd(0, 0, 0, 0, 0, 1, 4, 4, 8, 7, 0, 0)
    with pytest.raises(PfrError, match="multiple of 8"):
        lib.pfr_dwconv2d_fwd(p, p, 0, p, 1, 1, 4, 4, 12, 7, 0, 0)
    with pytest.raises(PfrError, match="not a device pointer"):
        lib.pfr_dwconv2d_fwd(p, p, 0, p, 0, 1, 4, 4, 8, 7, 0, 0)
    with pytest.raises(PfrError, match="not a device pointer"):
        lib.pfr_dwconv2d_wgrad(p, p, p, p, 0, 0, 1, 4, 4, 8, 7, 0, 0)
    with pytest.raises(PfrError, match="not a device pointer"):
        lib.pfr_layer_scale_fwd(p, p, 0, p, p, 0, 1, 4, 8, 0)
    with pytest.raises(PfrError, match="not a device pointer"):
        lib.pfr_layer_scale_bwd(p, p, p, 0, p, p, 0, 0, 1, 4, 8, 0, 0)
    with pytest.raises(PfrError, match="null pointer"):
        lib.pfr_layer_scale_bwd(0, 0, 0, 0, 0, 0, 0, 0, 1, 4, 8, 0, 0)


def test_block_setting_forms_and_cached_probabilities():
    """torchvision's CNBlockConfig objects (attributes) and plain tuples both describe the stages; the probability tensor of
    _draw_sd is built once per device and not at all in eval mode"""
    import types
    import pets_face_recognition_amd.models as M
    cfgs = [types.SimpleNamespace(input_channels=8, out_channels=16, num_layers=1),
            types.SimpleNamespace(input_channels=16, out_channels=None, num_layers=2)]
    a = M.ConvNeXt(block_setting=cfgs, num_classes=4, stochastic_depth_prob=0.2)
    b = M.ConvNeXt(block_setting=[(8, 16, 1), (16, None, 2)], num_classes=4)
    assert a.dims == b.dims == (8, 16) and a.depths == b.depths == (1, 2)
    assert list(a.state_dict()) == list(b.state_dict())
    a.eval()
    a._draw_sd(2, "cpu")
    assert a._sd_p == {}
    a.train()
    a._draw_sd(2, "cpu")
    p = a._sd_p["cpu"]
    a._draw_sd(3, "cpu")
    assert a._sd_p["cpu"] is p and p.tolist() == pytest.approx(a.sd_probs)
