"""models/_vit_engine.ViTEngine on the device against the CPU module (which tests/test_vit_host.py pins to an independent fp64
restatement): forward / backward in fp32 and bf16 at 17, 257 and 197 tokens, the engine contracts the optimizers and the Trainer rely
on, eval mode, the refused dropout, the full-width ViT-B/16 forward and three training steps of the ViT-B/16 + ArcFace model.

Net of the small tests: 192 wide, 3 heads (head_dim 64), MLP 384, 2 layers.  LayerNorm parameters, biases, the class token and the
zero-initialised `heads.head` are moved off their init before comparing: with the zero head every gradient upstream of it is zero
and a broken backward would pass."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
NET = dict(num_layers=2, num_heads=3, hidden_dim=192, mlp_dim=384, num_classes=64)
# bounds of test_swin_fwd_bwd_vs_torch_restatement (the TOL table of tests/test_convnext_gpu.py): embeddings, worst per-tensor
# gradient, cosine of the flat gradient
TOL = {torch.float32: (1e-3, 5e-3, 0.99999), torch.bfloat16: (5e-2, 1.5e-1, 0.99)}
SHAPES = [(4, 64, 16, 2), (2, 128, 8, 2), (2, 224, 16, 1)]       # (batch, image size, patch, layers): 17, 257 and 197 tokens
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():            # LayerNorm parameters, biases and the class token off their trivial init
            if p.dim() == 1 or n == "class_token":
                p.add_(torch.randn(p.shape, generator=g) * 0.1)
        head = m.heads if isinstance(m.heads, torch.nn.Linear) else m.heads[len(m.heads) - 1]
        head.weight.copy_(torch.randn(head.weight.shape, generator=g) * 0.05)


def _pair(dtype, image_size=64, patch=16, seed=21, **over):
    """(CPU module, device module with the same weights)"""
    import pets_face_recognition_amd.models as M
    torch.manual_seed(seed)
    kw = dict(NET, image_size=image_size, patch_size=patch, **over)
    ref = M.VisionTransformer(**kw)
    _perturb(ref, seed)
    hip = M.VisionTransformer(compute_dtype=dtype, **kw)
    hip.load_state_dict(ref.state_dict())
    return ref, hip.to(DEV)


def _input(seed=5, n=4, hw=64):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, hw, hw, generator=g)


def _compare_grads(hip, ref, dtype):
    tol_e, tol_g, tol_cos = TOL[dtype]
    rp = dict(ref.named_parameters())
    hp = dict(hip.named_parameters())
    assert set(hp) == set(rp)
    worst = ("", 0.0)
    fh, fr = [], []
    for n, p in hp.items():
        assert p.grad is not None and rp[n].grad is not None, n          # no parameter is left out
        assert rp[n].grad.norm() > 0, n
        r = rel(p.grad, rp[n].grad)
        fh.append(p.grad.double().cpu().flatten()); fr.append(rp[n].grad.double().flatten())
        if r > worst[1]:
            worst = (n, r)
    cos = F.cosine_similarity(torch.cat(fh), torch.cat(fr), dim=0).item()
    print(f"{dtype}: worst gradient {worst[0]} {worst[1]:.3e}, cosine {cos:.7f}")
    assert cos > tol_cos, cos
    assert worst[1] < tol_g, worst


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,hw,patch,layers", SHAPES, ids=["S17", "S257", "S197"])
def test_vit_fwd_bwd_vs_cpu_module(n, hw, patch, layers, dtype):
    ref, hip = _pair(dtype, image_size=hw, patch=patch, num_layers=layers)
    assert ref.seq_length == (hw // patch) ** 2 + 1
    ref.train(); hip.train()
    x = _input(n=n, hw=hw)
    e_ref = ref(x)
    e_ref.square().sum().backward()
    e = hip(x.to(DEV))
    e.square().sum().backward()
    torch.cuda.synchronize()
    err = rel(e, e_ref.detach())
    print(f"S={ref.seq_length} {dtype}: embedding rel err {err:.3e}")
    assert err < TOL[dtype][0]
    assert {"class_token", "encoder.pos_embedding"} <= {k for k, p in hip.named_parameters() if p.grad is not None}
    _compare_grads(hip, ref, dtype)


def test_vit_engine_contracts():
    from pets_face_recognition_amd.optim import FusedAdamW
    dtype = torch.float32
    ref, hip = _pair(dtype)
    keys = list(ref.state_dict())
    hip.train()
    x = _input().to(DEV)
    hip(x).square().sum().backward()
    torch.cuda.synchronize()
    eng = hip.hip_engine()
    # parameters (and their gradients) are views of the flat buffers
    lo, hi = eng.master.data_ptr(), eng.master.data_ptr() + 4 * eng.master.numel()
    glo, ghi = eng.grad.data_ptr(), eng.grad.data_ptr() + 4 * eng.grad.numel()
    for n, p in hip.named_parameters():
        assert lo <= p.data_ptr() < hi, n
        assert glo <= p.grad.data_ptr() < ghi, n
    # two backward passes without zero_grad: twice the gradient
    g1 = {n: p.grad.clone() for n, p in hip.named_parameters()}
    hip(x).square().sum().backward()
    torch.cuda.synchronize()
    for n, p in hip.named_parameters():
        assert rel(p.grad, 2 * g1[n]) < 1e-6, n
    # a second batch size builds a second plan; the first still replays
    n_plans = len(eng.plans)
    with torch.no_grad():
        e_a = hip(x).clone()
        x2 = _input(seed=9, n=2).to(DEV)
        e_b = hip(x2)
        assert len(eng.plans) > n_plans
        assert rel(e_b, ref(x2.cpu())) < 1e-3
        assert torch.equal(hip(x), e_a)
    # an optimizer step moves every parameter and shows in the next forward (the compute-dtype shadow and the conv layout are refreshed)
    opt = FusedAdamW(hip.parameters(), lr=1e-2)
    opt.zero_grad()
    hip(x).square().sum().backward()
    before = {n: p.detach().clone() for n, p in hip.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    assert all(not torch.equal(before[n], p.detach()) for n, p in hip.named_parameters())
    assert all(lo <= p.data_ptr() < hi for p in hip.parameters())
    # the state dict round-trips with unchanged keys
    sd = hip.state_dict()
    assert list(sd) == keys
    ref.load_state_dict({k: v.cpu() for k, v in sd.items()})
    with torch.no_grad():
        e2 = hip(x)
        assert rel(e2, ref(x.cpu())) < 1e-3
        assert rel(e2, e_a) > 1e-3
    hip.load_state_dict(sd)
    with torch.no_grad():
        assert torch.equal(hip(x), e2)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_vit_eval_mode_matches_cpu_and_builds_no_graph(dtype):
    ref, hip = _pair(dtype)
    ref.eval(); hip.eval()
    x = _input(seed=8)
    e = hip(x.to(DEV))                      # grad mode on: still the inference plan
    torch.cuda.synchronize()
    assert not e.requires_grad and e.grad_fn is None
    assert all(not k[3] for k in hip.hip_engine().plans)         # (N, H, W, with_backward, ...)
    with torch.no_grad():
        assert rel(e, ref(x)) < TOL[dtype][0]


def test_vit_dropout_in_training_is_refused_and_heads_forms():
    from pets_face_recognition_amd._hip import PfrError
    import pets_face_recognition_amd.models as M
    kw = dict(NET, image_size=64, patch_size=16, compute_dtype=torch.float32)
    x = _input().to(DEV)
    for drop in (dict(attention_dropout=0.1), dict(dropout=0.1)):
        m = M.VisionTransformer(**kw, **drop).to(DEV).train()
        with pytest.raises(PfrError, match="Dropout"):
            m(x)
        m.eval()
        assert tuple(m(x).shape) == (4, 64)                       # eval mode: dropout is the identity
    # head_dim 80 (vit_h_14's): no attention kernel
    m = M.VisionTransformer(image_size=64, patch_size=16, num_layers=1, num_heads=2, hidden_dim=160, mlp_dim=320, num_classes=8).to(DEV)
    with pytest.raises(PfrError, match="no attention kernel"):
        m(x)
    # `heads` as a bare Linear (the FE line) and as a Sequential ending in the Linear
    torch.manual_seed(3)
    ref = M.VisionTransformer(**dict(kw, compute_dtype=None))
    ref.heads = torch.nn.Linear(192, 32)
    _perturb(ref, 3)
    for form in ("linear", "sequential"):
        hip = M.VisionTransformer(**kw)
        hip.heads = torch.nn.Linear(192, 32)
        hip.load_state_dict(ref.state_dict())
        if form == "sequential":
            hip.heads = torch.nn.Sequential(torch.nn.Identity(), hip.heads)
        hip = hip.to(DEV).train()
        ref.zero_grad()
        e_ref = ref(x.cpu())
        e_ref.square().sum().backward()
        e = hip(x)
        e.square().sum().backward()
        torch.cuda.synchronize()
        assert rel(e, e_ref.detach()) < 1e-3
        hw = hip.heads.weight if form == "linear" else hip.heads[1].weight
        assert rel(hw.grad, ref.heads.weight.grad) < 5e-3
    # another image size than the position embedding's
    with pytest.raises(ValueError, match="pos_embedding was built for"):
        hip(_input(hw=32).to(DEV))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_vit_b_16_full_width_forward(dtype):
    """vit_b_16 with heads = Linear(768, 512) at [2,3,224,224], forward only"""
    import pets_face_recognition_amd.models as M
    torch.manual_seed(4)
    ref = M.vit_b_16()
    ref.heads = torch.nn.Linear(768, 512)
    _perturb(ref, 4)
    hip = M.vit_b_16(compute_dtype=dtype)
    hip.heads = torch.nn.Linear(768, 512)
    hip.load_state_dict(ref.state_dict())
    hip = hip.to(DEV).eval()
    ref.eval()
    x = _input(seed=3, n=2, hw=224)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with torch.no_grad():
        e_ref = ref(x)
        e = hip(x.to(DEV))
    torch.cuda.synchronize()
    err = rel(e, e_ref)
    print(f"ViT-B/16 {dtype} embedding rel err {err:.3e}")
    assert tuple(e.shape) == (2, 512) and err < TOL[dtype][0]


def test_vit_b_16_arcface_three_training_steps_match_cpu():
    """The model and head of configs/synthetic/fe_vit_b_16_mi355x.py (vit_b_16, heads = Linear(768, 512), ArcFace + focal loss,
    AdamW with the backbone / heads / margin groups) at B = 8 in fp32: three steps on the device (FusedAdamW) reproduce the loss
    trace of the CPU module (torch.optim.AdamW).  The ConvNeXt and MobileNet device tests only ask their traces to be finite; the
    bound here is the fp32 embedding bound of the TOL table, 1e-3 relative per step: the loss is a smooth function of embeddings
    that agree to that bound, and AdamW's steps (|Δw| <= lr = 1e-3 per weight and step) cannot amplify the fp32 rounding
    differences of the gradients beyond it in three steps."""
    import pets_face_recognition_amd.models as M
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    from pets_face_recognition_amd.optim import FusedAdamW
    C, B = 100, 8
    torch.set_num_threads(min(16, os.cpu_count() or 1))

    def build(dtype):
        torch.manual_seed(12)
        m = M.vit_b_16(**({} if dtype is None else {"compute_dtype": dtype}))
        m.heads = torch.nn.Linear(768, 512)
        ml = SoftmaxBasedMetricLearning(model=m, num_class=C, embedding_size=512, is_focal=True, arc_margin=True)
        return ml

    def groups(ml, base=1e-3):
        p1 = [p for n, p in ml.module.named_parameters() if "heads" not in n]
        p2 = [p for n, p in ml.module.named_parameters() if "heads" in n]
        return [{"lr": base / 2, "params": p1}, {"lr": base, "params": p2},
                {"lr": base, "params": list(ml.add_margin.parameters()), "weight_decay": 1e-4}]

    ref = build(None)
    hip = build(torch.float32)
    hip.load_state_dict(ref.state_dict())
    if hasattr(hip.add_margin, "compute_dtype"):
        hip.add_margin.compute_dtype = torch.float32
    hip = hip.to(DEV)
    ref.train(); hip.train()
    o_ref = torch.optim.AdamW(groups(ref), 1e-3, weight_decay=0.05)
    o_hip = FusedAdamW(groups(hip), 1e-3, weight_decay=0.05)
    g = torch.Generator().manual_seed(2)
    trace_ref, trace_hip = [], []
    for step in range(3):
        x = torch.rand(B, 3, 224, 224, generator=g)
        y = torch.randint(0, C, (B,), generator=g)
        o_ref.zero_grad()
        l_ref = ref(x, y)["loss"]
        l_ref.backward()
        o_ref.step()
        o_hip.zero_grad()
        l_hip = hip(x.to(DEV), y.to(DEV))["loss"]
        l_hip.backward()
        o_hip.step()
        trace_ref.append(l_ref.item()); trace_hip.append(l_hip.item())
    torch.cuda.synchronize()
    print("loss trace cpu", trace_ref, "device", trace_hip)
    assert trace_ref[0] != trace_ref[2]
    for a, b in zip(trace_hip, trace_ref):
        assert abs(a - b) <= 1e-3 * abs(b), (trace_hip, trace_ref)
