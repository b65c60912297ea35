"""Vision Transformer on the host: torchvision's parameter counts and state-dict layout, the CPU module against an independent fp64
restatement written out here (explicit softmax(QKᵀ·scale)·V, F.layer_norm, F.gelu — no nn.MultiheadAttention), the two `heads` forms,
the pretrained flag, the synthetic CPU config through the Controller / Trainer path of main.py, and the argument checks of the new
C-ABI entries (no device work)."""
import ctypes
import math
import os

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTH = os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic")
TINY = dict(image_size=32, patch_size=8, num_layers=2, num_heads=3, hidden_dim=192, mlp_dim=384)


def _count(m):
    return sum(p.numel() for p in m.parameters())


def test_parameter_counts_are_torchvisions():
    import pets_face_recognition_amd.models as M
    with torch.device("meta"):
        b16, b32, l16 = M.vit_b_16(), M.vit_b_32(), M.vit_l_16()
    assert _count(b16) == 86_567_656
    assert _count(b32) == 88_224_232
    assert _count(l16) == 304_326_632
    with torch.device("meta"):
        s16, t16 = M.vit_s_16(), M.vit_t_16()
    assert (s16.hidden_dim, s16.num_heads, s16.mlp_dim, len(s16.encoder.layers)) == (384, 6, 1536, 12)
    assert (t16.hidden_dim, t16.num_heads, t16.mlp_dim, len(t16.encoder.layers)) == (192, 3, 768, 12)
    assert s16.hidden_dim // s16.num_heads == t16.hidden_dim // t16.num_heads == 64


def _torchvision_keys(layers=12, D=768, mlp=3072, S=197, patch=16, num_classes=1000):
    """torchvision.models.vit_b_16().state_dict() keys → shapes, written out"""
    k = {"class_token": (1, 1, D), "conv_proj.weight": (D, 3, patch, patch), "conv_proj.bias": (D,),
         "encoder.pos_embedding": (1, S, D)}
    for i in range(layers):
        p = f"encoder.layers.encoder_layer_{i}."
        k[p + "ln_1.weight"] = (D,)
        k[p + "ln_1.bias"] = (D,)
        k[p + "self_attention.in_proj_weight"] = (3 * D, D)
        k[p + "self_attention.in_proj_bias"] = (3 * D,)
        k[p + "self_attention.out_proj.weight"] = (D, D)
        k[p + "self_attention.out_proj.bias"] = (D,)
        k[p + "ln_2.weight"] = (D,)
        k[p + "ln_2.bias"] = (D,)
        k[p + "mlp.0.weight"] = (mlp, D)
        k[p + "mlp.0.bias"] = (mlp,)
        k[p + "mlp.3.weight"] = (D, mlp)
        k[p + "mlp.3.bias"] = (D,)
    k["encoder.ln.weight"] = (D,)
    k["encoder.ln.bias"] = (D,)
    k["heads.head.weight"] = (num_classes, D)
    k["heads.head.bias"] = (num_classes,)
    return k


def test_state_dict_keys_shapes_and_init_are_torchvisions():
    import pets_face_recognition_amd.models as M
    m = M.vit_b_16()
    want = _torchvision_keys()
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert len(got) == 152
    assert got == want
    assert got["encoder.layers.encoder_layer_0.self_attention.in_proj_weight"] == (2304, 768)
    assert got["encoder.pos_embedding"] == (1, 197, 768)
    assert got["conv_proj.weight"] == (768, 3, 16, 16)
    assert list(m.state_dict())[:4] == ["class_token", "conv_proj.weight", "conv_proj.bias", "encoder.pos_embedding"]
    # a checkpoint with those keys loads strictly
    g = torch.Generator().manual_seed(0)
    small = M.VisionTransformer(num_classes=10, **TINY)
    sd = {k: torch.randn(v.shape, generator=g) for k, v in small.state_dict().items()}
    small.load_state_dict(sd, strict=True)
    # details of the definition and torchvision's initialisation
    blk = m.encoder.layers.encoder_layer_0
    assert blk.ln_1.eps == blk.ln_2.eps == m.encoder.ln.eps == 1e-6
    assert isinstance(blk.mlp[1], torch.nn.GELU) and blk.mlp[1].approximate == "none"
    assert blk.self_attention.dropout == 0.0 and blk.dropout.p == 0.0 and m.encoder.dropout.p == 0.0
    assert torch.all(m.class_token == 0) and torch.all(m.heads.head.weight == 0) and torch.all(m.heads.head.bias == 0)
    assert abs(m.encoder.pos_embedding.std().item() - 0.02) < 5e-4                   # 151 296 draws of N(0, 0.02)
    std = math.sqrt(1 / (3 * 16 * 16))
    w = m.conv_proj.weight
    assert abs(w.std().item() - std) < 0.02 * std and w.abs().max().item() <= 2.0   # trunc-normal, cut at ±2 = ±55 std; 589 824 draws
    assert torch.all(m.conv_proj.bias == 0)
    assert m.seq_length == 197 and M.vit_b_32(num_classes=2).seq_length == 50


def _restate(m, x):
    """the forward of models/vit.py in fp64 from the parameters alone"""
    P = dict(m.named_parameters())
    D, heads, p = m.hidden_dim, m.num_heads, m.patch_size
    hd = D // heads
    B = x.shape[0]
    # patch embedding as an explicit unfold + matmul
    patches = F.unfold(x, kernel_size=p, stride=p).transpose(1, 2)                   # [B, n, 3*p*p] in (c, kh, kw) order
    t = patches @ P["conv_proj.weight"].reshape(D, -1).t() + P["conv_proj.bias"]
    t = torch.cat([P["class_token"].expand(B, 1, D), t], dim=1) + P["encoder.pos_embedding"]
    S = t.shape[1]
    for i in range(len(m.encoder.layers)):
        q = f"encoder.layers.encoder_layer_{i}."
        y = F.layer_norm(t, (D,), P[q + "ln_1.weight"], P[q + "ln_1.bias"], 1e-6)
        qkv = y @ P[q + "self_attention.in_proj_weight"].t() + P[q + "self_attention.in_proj_bias"]
        qq, kk, vv = (z.reshape(B, S, heads, hd).permute(0, 2, 1, 3) for z in qkv.split(D, dim=-1))
        a = torch.softmax(qq @ kk.transpose(-1, -2) * (1.0 / math.sqrt(hd)), dim=-1) @ vv
        a = a.permute(0, 2, 1, 3).reshape(B, S, D)
        t = t + a @ P[q + "self_attention.out_proj.weight"].t() + P[q + "self_attention.out_proj.bias"]
        y = F.layer_norm(t, (D,), P[q + "ln_2.weight"], P[q + "ln_2.bias"], 1e-6)
        h = F.gelu(y @ P[q + "mlp.0.weight"].t() + P[q + "mlp.0.bias"])
        t = t + h @ P[q + "mlp.3.weight"].t() + P[q + "mlp.3.bias"]
    c = F.layer_norm(t[:, 0], (D,), P["encoder.ln.weight"], P["encoder.ln.bias"], 1e-6)
    return c @ P["heads.head.weight"].t() + P["heads.head.bias"]


def test_cpu_module_matches_fp64_restatement():
    """Bounds of tests/test_convnext_host.py against its independent implementation: output within 1e-5 relative, every parameter
    gradient within 1e-4 relative (both sides fp64; measured here: 8e-16 and 2e-15)."""
    import pets_face_recognition_amd.models as M
    torch.manual_seed(7)
    m = M.VisionTransformer(num_classes=16, **TINY).double()
    with torch.no_grad():
        for n, p in m.named_parameters():            # biases, LayerNorm parameters, class token and the zero head off their init
            if p.dim() == 1 or n == "class_token":
                p.add_(torch.randn_like(p) * 0.1)
        m.heads.head.weight.normal_(std=0.05)
    x = torch.randn(3, 3, 32, 32, dtype=torch.float64)
    out = m(x)
    out.square().sum().backward()
    got = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    ref = _restate(m, x)
    ref.square().sum().backward()
    e = ((out - ref).norm() / ref.norm()).item()
    print(f"output rel err {e:.3e}")
    assert tuple(out.shape) == (3, 16) and e < 1e-5
    worst = 0.0
    for n, p in m.named_parameters():
        assert p.grad is not None and p.grad.norm() > 0, n
        r = ((got[n] - p.grad).norm() / p.grad.norm()).item()
        worst = max(worst, r)
        assert r < 1e-4, (n, r)
    print(f"worst gradient rel err {worst:.3e}")


def test_heads_forms_and_input_size():
    import pets_face_recognition_amd.models as M
    from pets_face_recognition_amd.models._vit_engine import _head_linear
    from pets_face_recognition_amd._hip import PfrError
    m = M.VisionTransformer(num_classes=10, **TINY)
    assert _head_linear(m.heads)[0] == "heads.head"
    x = torch.randn(2, 3, 32, 32)
    assert tuple(m(x).shape) == (2, 10)
    m.heads = torch.nn.Linear(192, 512)                                 # the FE line
    assert _head_linear(m.heads) == ("heads", m.heads)
    assert tuple(m(x).shape) == (2, 512)
    assert "heads.weight" in m.state_dict()
    m.heads = torch.nn.Sequential(torch.nn.Identity(), torch.nn.Linear(192, 7))
    assert _head_linear(m.heads) == ("heads.1", m.heads[1])
    assert tuple(m(x).shape) == (2, 7)
    with pytest.raises(PfrError, match="only Linear is its last module"):
        _head_linear(torch.nn.Sequential(torch.nn.Linear(192, 64), torch.nn.Tanh(), torch.nn.Linear(64, 7)))
    # no position interpolation: another image size is a plain error
    with pytest.raises(ValueError, match="pos_embedding was built for"):
        m(torch.randn(2, 3, 64, 64))


def test_pretrained_flag_is_refused_like_the_other_factories():
    """`pretrained=True` raises the UserWarning of models/resnet._no_pretrained, as every factory of the package does"""
    import pets_face_recognition_amd.models as M
    with pytest.warns(UserWarning, match="pretrained=True ignored"):
        M.vit_t_16(pretrained=True, num_classes=4, **TINY)


def test_fe_vit_cpu_config_trains_two_steps(tmp_path, monkeypatch):
    """configs/synthetic/fe_vit_cpu.py through main.py's path: config wrapper → Controller → Trainer.fit"""
    import pets_face_recognition_amd as pfr
    from pets_face_recognition_amd.engine import Trainer
    from pets_face_recognition_amd.engine.controller import Controller
    from pets_face_recognition_amd.utils import get_dict_wrapper
    pfr.install_reference_aliases()
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("PFR_LIMIT_TRAIN_BATCHES", "2")
    cfg = get_dict_wrapper(os.path.join(SYNTH, "fe_vit_cpu.py"))
    torch.manual_seed(11)
    ctrl = Controller(cfg)
    import pets_face_recognition_amd.models as M
    vit = [m for m in ctrl.modules() if isinstance(m, M.VisionTransformer)]
    assert len(vit) == 1 and isinstance(vit[0].heads, torch.nn.Linear) and vit[0].heads.out_features == 512
    opt = ctrl.configure_optimizers()[0][0]
    assert isinstance(opt, torch.optim.AdamW)
    # the 'fc' parameter group of the reference's split is `heads`: a group of its own at the full base rate
    heads = list(vit[0].heads.parameters())
    groups = [g for g in opt.param_groups if len(g["params"]) == 2 and g["params"][0] is heads[0] and g["params"][1] is heads[1]]
    assert len(groups) == 1 and len(opt.param_groups) == 3
    assert groups[0]["lr"] == 2 * opt.param_groups[0]["lr"]
    before = [p.detach().clone() for p in ctrl.parameters()]
    t = Trainer(gpus=0, max_epochs=1, check_val_every_n_epoch=100, prefetch_batches=0, log_every_n_steps=1, **cfg.trainer_kwargs)
    t.fit(ctrl)
    assert t.global_step == 2 and len(t.loss_history) == 2
    assert all(math.isfinite(float(v)) for v in t.loss_history), t.loss_history
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, ctrl.parameters()))


def test_new_entries_are_declared_and_report_argument_errors():
    """unsupported shapes, null and host pointers: an error code (PfrError through the binding), never a launch"""
    from pets_face_recognition_amd._hip import lib, PfrError
    syms = lib.symbols()
    for name in ("pfr_mha_fwd", "pfr_mha_bwd", "pfr_mha_supported", "pfr_vit_tokens_fwd", "pfr_vit_tokens_bwd", "pfr_vit_cls_fwd",
                 "pfr_vit_cls_bwd"):
        assert name in syms
    assert lib.pfr_plan_thunk_index(b"pfr_mha_fwd") >= 0 and lib.pfr_plan_thunk_index(b"pfr_mha_bwd") >= 0
    for dt in (0, 1):
        for S in (1, 50, 64, 65, 197, 257):
            assert lib.pfr_mha_supported(dt, S, 12, 64) == 1
        assert lib.pfr_mha_supported(dt, 258, 12, 64) == 0
        assert lib.pfr_mha_supported(dt, 0, 12, 64) == 0
        assert lib.pfr_mha_supported(dt, 197, 16, 80) == 0                  # vit_h_14
        assert lib.pfr_mha_supported(dt, 197, 12, 32) == 0
    assert lib.pfr_mha_supported(2, 197, 12, 64) == 0                       # int8
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    with pytest.raises(PfrError, match="unsupported shape"):
        lib.pfr_mha_fwd(p, p, p, 0, 1, 258, 1, 64, 0.125, 0)
    with pytest.raises(PfrError, match="unsupported shape"):
        lib.pfr_mha_fwd(p, p, p, 1, 1, 16, 1, 80, 0.125, 0)
    with pytest.raises(PfrError, match="unsupported shape"):
        lib.pfr_mha_bwd(p, p, p, p, p, 0, 1, 16, 1, 32, 0.125, 0)
    with pytest.raises(PfrError, match="null pointer"):
        lib.pfr_mha_fwd(0, 0, 0, 0, 1, 4, 1, 64, 0.125, 0)
    with pytest.raises(PfrError, match="null pointer"):
        lib.pfr_mha_bwd(p, p, p, 0, p, 0, 1, 4, 1, 64, 0.125, 0)
    with pytest.raises(PfrError, match="multiple of 8"):
        lib.pfr_vit_tokens_fwd(p, p, p, p, 1, 1, 5, 12, 0)
    with pytest.raises(PfrError, match="null pointer"):
        lib.pfr_vit_tokens_bwd(0, 0, 0, 0, 0, 1, 5, 8, 0)
    with pytest.raises(PfrError, match="null pointer"):
        lib.pfr_vit_cls_fwd(0, 0, 0, 1, 5, 8, 0)
