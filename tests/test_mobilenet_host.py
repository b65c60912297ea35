"""MobileNetV2 on the host: torchvision's state-dict layout and channel tables, the reference's head swap, the CPU module against an
independent implementation (Hugging Face MobileNetV2Model, fixture written by tools/make_mobilenet_golden.py), and the argument
checks of the new C-ABI entries (no device work)."""
import ctypes
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden")

# torchvision's t, c, n, s table expanded by hand: (inp, oup, stride, t) per block at width 1.0
BLOCKS = [(32, 16, 1, 1),
          (16, 24, 2, 6), (24, 24, 1, 6),
          (24, 32, 2, 6), (32, 32, 1, 6), (32, 32, 1, 6),
          (32, 64, 2, 6), (64, 64, 1, 6), (64, 64, 1, 6), (64, 64, 1, 6),
          (64, 96, 1, 6), (96, 96, 1, 6), (96, 96, 1, 6),
          (96, 160, 2, 6), (160, 160, 1, 6), (160, 160, 1, 6),
          (160, 320, 1, 6)]


def _bn(k, prefix, C):
    k[prefix + ".weight"] = (C,)
    k[prefix + ".bias"] = (C,)
    k[prefix + ".running_mean"] = (C,)
    k[prefix + ".running_var"] = (C,)
    k[prefix + ".num_batches_tracked"] = ()


def _torchvision_keys(num_classes=1000, head="classifier.1"):
    """torchvision.models.mobilenet_v2().state_dict() keys → shapes, written out"""
    k = {"features.0.0.weight": (32, 3, 3, 3)}
    _bn(k, "features.0.1", 32)
    for i, (inp, oup, _s, t) in enumerate(BLOCKS, start=1):
        p = f"features.{i}.conv."
        hidden = inp * t
        j = 0
        if t != 1:
            k[p + "0.0.weight"] = (hidden, inp, 1, 1)
            _bn(k, p + "0.1", hidden)
            j = 1
        k[p + f"{j}.0.weight"] = (hidden, 1, 3, 3)
        _bn(k, p + f"{j}.1", hidden)
        k[p + f"{j + 1}.weight"] = (oup, hidden, 1, 1)
        _bn(k, p + f"{j + 2}", oup)
    k["features.18.0.weight"] = (1280, 320, 1, 1)
    _bn(k, "features.18.1", 1280)
    k[head + ".weight"] = (num_classes, 1280)
    k[head + ".bias"] = (num_classes,)
    return k


def _random_sd(want, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.randn(s, generator=g) if s != () else torch.tensor(7)) for k, s in want.items()}


def test_state_dict_keys_shapes_and_parameter_count_are_torchvisions():
    import pets_face_recognition_amd.models as M
    m = M.mobilenet_v2()
    want = _torchvision_keys()
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    assert list(m.state_dict()) == list(want)       # and in torchvision's order
    assert sum(p.numel() for p in m.parameters()) == 3504872
    assert sum(p.numel() for p in m.classifier.parameters()) == 1281000
    assert m.last_channel == 1280
    sd = _random_sd(want)
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.features[2].conv[1][0].weight, sd["features.2.conv.1.0.weight"])
    assert int(m.features[0][1].num_batches_tracked) == 7
    # details of the definition
    fresh = M.mobilenet_v2(num_classes=8)
    bn = fresh.features[3].conv[0][1]
    assert bn.eps == 1e-5 and bn.momentum == 0.1
    assert [b.use_res_connect for b in fresh.features[1:18]] == [s == 1 and i == o for i, o, s, _t in BLOCKS]
    assert len(fresh.features[1].conv) == 3 and len(fresh.features[2].conv) == 4          # the t = 1 block has no expand conv
    assert isinstance(fresh.classifier[0], torch.nn.Dropout) and fresh.classifier[0].p == 0.2
    assert abs(fresh.classifier[1].weight.std().item() - 0.01) < 1e-3 and torch.all(fresh.classifier[1].bias == 0)
    w = fresh.features[18][0].weight      # kaiming-normal, fan-out = 1280: std = sqrt(2 / 1280); 409600 weights
    assert abs(w.std().item() - (2 / 1280) ** 0.5) < 0.02 * (2 / 1280) ** 0.5
    assert torch.all(bn.weight == 1) and torch.all(bn.bias == 0)


def test_reference_head_swap_loads_strictly_and_embeds_to_512():
    import pets_face_recognition_amd.models as M
    m = M.mobilenet_v2(pretrained=False)
    m.classifier = torch.nn.Sequential(torch.nn.Linear(m.last_channel, 512))
    want = _torchvision_keys(512, head="classifier.0")
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    m.load_state_dict(_random_sd(want, 1), strict=True)
    m.eval()
    with torch.no_grad():
        assert tuple(m(torch.randn(2, 3, 64, 64)).shape) == (2, 512)


def test_pretrained_flag_warns():
    import pets_face_recognition_amd.models as M
    with pytest.warns(UserWarning, match="pretrained=True ignored"):
        M.mobilenet_v2(pretrained=True, inverted_residual_setting=[[1, 16, 1, 1]], num_classes=4)


def test_make_divisible_and_width_tables():
    import pets_face_recognition_amd.models as M
    from pets_face_recognition_amd.models.mobilenet import _make_divisible
    assert [_make_divisible(v) for v in (1, 8, 11, 12, 16, 33.6, 44.8, 100)] == [8, 8, 16, 16, 16, 32, 48, 104]
    assert _make_divisible(10, 8) == 16 and _make_divisible(1.5 * 32, 8) == 48      # 8 would be more than 10 % below 10
    assert _make_divisible(90, 64) == 128 and _make_divisible(23, 4) == 24

    def table(m):
        return [m.features[0][0].out_channels] + [b.out_channels for b in m.features[1:-1]], m.last_channel

    half = [16, 8, 16, 16, 16, 16, 16, 32, 32, 32, 32, 48, 48, 48, 80, 80, 80, 160]
    big = [48, 24, 32, 32, 48, 48, 48, 88, 88, 88, 88, 136, 136, 136, 224, 224, 224, 448]
    assert table(M.mobilenet_v2(width_mult=0.5, num_classes=4)) == (half, 1280)
    assert table(M.mobilenet_v2(width_mult=1.4, num_classes=4)) == (big, 1792)
    assert table(M.mobilenet_v2(num_classes=4)) == ([32] + [o for _i, o, _s, _t in BLOCKS], 1280)


def test_new_entries_are_declared_and_plannable():
    from pets_face_recognition_amd._hip import lib
    protos = lib.symbols()
    launches = ["pfr_dwconv3_fwd", "pfr_dwconv3_dgrad", "pfr_dwconv3_wgrad", "pfr_bn_act_clamp", "pfr_bn_bwd_reduce_clamp",
                "pfr_bn_bwd_apply_clamp"]
    for name in launches + ["pfr_dwconv3_rows_per_part", "pfr_dwconv3_wgrad_parts"]:
        assert name in protos, name
    for name in launches:
        assert lib.pfr_plan_thunk_index(name.encode()) >= 0, name
    assert protos["pfr_dwconv3_fwd"][2] == ["x", "w", "y", "dtype", "N", "H", "W", "C", "stride", "pro_scale", "pro_shift", "pro_hi",
                                            "stats_part", "stream"]
    assert protos["pfr_dwconv3_fwd"][1][11] is ctypes.c_float and protos["pfr_bn_act_clamp"][1][4] is ctypes.c_float


def test_new_entries_report_argument_errors():
    """stride 3, a channel count off the 16-byte chunk, null and host pointers: an error code (PfrError through the binding), never a
    launch — the geometry checks come first, so none of this needs a device"""
    from pets_face_recognition_amd._hip import lib, PfrError
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    with pytest.raises(PfrError, match="stride 1 and 2"):
        lib.pfr_dwconv3_fwd(p, p, p, 0, 1, 4, 4, 8, 3, 0, 0, 0.0, 0, 0)
    with pytest.raises(PfrError, match="stride 1 and 2"):
        lib.pfr_dwconv3_dgrad(p, p, p, 0, 1, 4, 4, 8, 3, 0)
    with pytest.raises(PfrError, match="stride 1 and 2"):
        lib.pfr_dwconv3_wgrad(p, p, p, p, 0, 1, 4, 4, 8, 0, 0, 0, 0.0, 0, 0)
    with pytest.raises(PfrError, match="multiple of 8"):
        lib.pfr_dwconv3_fwd(p, p, p, 1, 1, 4, 4, 12, 1, 0, 0, 0.0, 0, 0)
    with pytest.raises(PfrError, match="multiple of 8"):
        lib.pfr_dwconv3_dgrad(p, p, p, 1, 1, 4, 4, 12, 2, 0)
    with pytest.raises(PfrError, match="null pointer"):
        lib.pfr_dwconv3_fwd(0, p, p, 0, 1, 4, 4, 8, 1, 0, 0, 0.0, 0, 0)
    with pytest.raises(PfrError, match="null pointer"):
        lib.pfr_dwconv3_wgrad(0, p, p, p, 0, 1, 4, 4, 8, 1, 0, 0, 0.0, 0, 0)
    with pytest.raises(PfrError, match="come together"):
        lib.pfr_dwconv3_fwd(p, p, p, 0, 1, 4, 4, 8, 1, p, 0, 6.0, 0, 0)
    with pytest.raises(PfrError, match="not a device pointer"):
        lib.pfr_dwconv3_fwd(p, p, p, 0, 1, 4, 4, 8, 1, 0, 0, 0.0, 0, 0)
    with pytest.raises(PfrError, match="null pointer"):
        lib.pfr_bn_act_clamp(0, p, p, p, 6.0, 0, 4, 8, 0)
    with pytest.raises(PfrError, match="!= 0"):
        lib.pfr_bn_act_clamp(p, p, p, p, 6.0, 1, 4, 12, 0)
    with pytest.raises(PfrError, match="mask_mode"):
        lib.pfr_bn_bwd_reduce_clamp(p, p, p, p, p, p, 6.0, 1, 0, 4, 8, p, 0)
    with pytest.raises(PfrError, match="mask_mode"):
        lib.pfr_bn_bwd_apply_clamp(p, p, p, p, p, 6.0, 3, p, 0, 4, 8, 0)
    with pytest.raises(PfrError, match="not a device pointer"):
        lib.pfr_bn_bwd_reduce_clamp(p, p, p, p, p, p, 6.0, 2, 0, 4, 8, p, 0)
    assert lib.pfr_dwconv3_rows_per_part(0, 1, 4, 4, 8, 3) == 0 and lib.pfr_dwconv3_wgrad_parts(0, 1, 4, 4, 8, 3) == 0
    assert lib.pfr_dwconv3_rows_per_part(1, 1, 4, 4, 12, 1) == 0
    # the row groups cover the output: ceil(rows / rpp) partial rows of rpp rows each
    for (N, H, W, C, s) in [(256, 112, 112, 96, 2), (3, 7, 7, 960, 1), (1, 1, 1, 16, 1)]:
        rpp = lib.pfr_dwconv3_rows_per_part(1, N, H, W, C, s)
        assert rpp >= 1 and lib.pfr_dwconv3_wgrad_parts(1, N, H, W, C, s) >= 1


def _fill_entry(rng, key, shape):
    """tools/make_mobilenet_golden.py:fill_entry"""
    if key.endswith("running_var") or (key.endswith("weight") and len(shape) == 1):
        return rng.uniform(0.5, 1.5, size=shape)
    if key.endswith("bias") or key.endswith("running_mean"):
        return rng.standard_normal(shape) * 0.1
    fan_in = int(np.prod(shape[1:]))
    return rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)


def _hf_to_ours(key):
    """Hugging Face MobileNetV2Model state-dict name → torchvision name (written out)"""
    t = key.split(".")
    if t[0] == "conv_stem":
        pre, part, kind, leaf = {"first_conv": "features.0.", "conv_3x3": "features.1.conv.0.", "reduce_1x1": "features.1.conv."}[t[1]], \
            t[1], t[2], t[3]
        first = 1
    elif t[0] == "layer":
        pre, part, kind, leaf = f"features.{int(t[1]) + 2}.conv.", t[2], t[3], t[4]
        pre += {"expand_1x1": "0.", "conv_3x3": "1.", "reduce_1x1": ""}[part]
        first = 2
    else:
        assert t[0] == "conv_1x1"
        return "features.18." + {"convolution": "0.", "normalization": "1."}[t[1]] + t[2]
    if part == "reduce_1x1":     # the project conv and its BatchNorm are plain members of the block's Sequential
        return pre + {"convolution": str(first), "normalization": str(first + 1)}[kind] + "." + leaf
    return pre + {"convolution": "0.", "normalization": "1."}[kind] + leaf


def test_cpu_module_matches_huggingface_mobilenet_v2():
    """eval mode, fp64, full width, [2,3,64,64]: the pooled 1280-d features within 1e-5 relative of the fixture"""
    import pets_face_recognition_amd.models as M
    G = np.load(os.path.join(GOLD, "mobilenet_v2_hf.npz"))
    keys = [str(k) for k in G["keys"]]
    shapes = [tuple(int(v) for v in str(s).split(",")) for s in G["shapes"]]
    m = M.mobilenet_v2(num_classes=4).double().eval()
    m.classifier = torch.nn.Identity()
    ours = m.state_dict()
    rng = np.random.default_rng(int(G["seed"]))
    names = []
    with torch.no_grad():
        for k, s in zip(keys, shapes):
            n = _hf_to_ours(k)
            names.append(n)
            assert tuple(ours[n].shape) == s, (k, n)
            ours[n].copy_(torch.from_numpy(_fill_entry(rng, k, s)))
    assert sorted(names) == sorted(k for k in ours if not k.endswith("num_batches_tracked")), "every entry is filled from the fixture"
    x = rng.standard_normal((2, 3, 64, 64))
    assert np.array_equal(x, G["x"])
    with torch.no_grad():
        pooled = m(torch.from_numpy(G["x"]))
    want = torch.from_numpy(G["pooled"])
    assert tuple(pooled.shape) == tuple(want.shape) == (2, 1280)
    e = ((pooled - want).norm() / want.norm()).item()
    print(f"pooled rel err {e:.3e}")
    assert e < 1e-5
