"""Pair losses on the device (csrc/pfr_pairloss.hip) against the float64 CPU implementation of the contract (losses/pair.py).

Kernel level, through the C-ABI wrappers: pfr_l2norm_fwd writes ê (and êᵀ) in the compute dtype, the oracle is evaluated in float64 ON
THOSE OPERAND BITS (the bf16-rounded ê in bf16 mode), so the only differences left are those of the kernels' own arithmetic.  Every
element of every case is compared (both losses are smooth on these inputs): l_i for every anchor, the scalar, every component of dê.

Bounds (derived, not tuned; ratios observed / bound are printed and recorded in profiles/pair_loss.txt):
  delta = D * 2^-24      a score is an fp32-accumulated dot product of two rows of length <= 1: D products, each partial sum <= 1
  eps   = slope * delta  the shift of a logit; slope = 1 / tau (supcon) or gamma * (1 + m) (circle: |gamma alpha| <= gamma (1 + m) + gamma)
  forward   l_i is a log-sum-exp (1-Lipschitz in the sup norm) minus a mean (supcon), or a softplus (1-Lipschitz) of the sum of two
            log-sum-exps (circle): |dl_i| <= 2 eps.  The scalar is a mean of l_i: the same bound.
  gradient  W_ij = (1 / A) f_i softmax_ij slope_ij (supcon: minus [j in P] / (|P| tau A), which can cancel to 0; U_ij is the sum of the
            two magnitudes, |W_ij| for circle).  A logit shift of eps moves a softmax weight by a factor in [e^-2eps, e^2eps] and
            f_i = sigma(z_i) by a factor within e^(2 eps) (d ln sigma / dz <= 1, |dz| <= 2 eps): relative 4 eps to first order.  Circle's
            slope_ij = gamma alpha_ij moves by gamma * delta absolutely, which moves W_ij by q_ij gamma delta with q = |d loss / d logit|
            (the pair's softmax weight, from the oracle).  The second product sums B terms in fp32 and G itself is a handful of fp32
            operations: (B + 8) * 2^-24 relative to sum_j |G_rj|.  With |ê_jd| <= 1, per component of row r:
              fp32:  E_r = (4 eps + (B + 8) 2^-24) sum_j (U_rj + U_jr) + gamma delta sum_j (q_rj + q_jr)
              bf16:  2^-8 sum_j |W_rj + W_jr| + E_r     (G rounded to bf16 for the MFMA: 2^-9 relative, half of what is allowed)
            all times the upstream gradient."""
import os
import sys

import pytest
import torch
import torch.nn as nn

from pets_face_recognition_amd.losses.pair import PairLoss, pair_loss_from_scores, pair_loss_torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SYNTH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pets-face-recognition_amd", "configs", "synthetic")
KINDS = {"supcon": dict(tau=0.1), "circle": dict(m=0.25, gamma=64.0)}
UP = 0.75          # the upstream gradient of every kernel-level case (a device scalar), so that none passes by ignoring it
RATIOS = {}        # (what, dtype) -> largest observed error / bound, printed by every test that updates it


def ops():
    from pets_face_recognition_amd._hip import ops as o
    return o


def slope_of(kind, p):
    return 1.0 / p["tau"] if kind == "supcon" else p["gamma"] * (1.0 + p["m"])


def layouts(B, seed):
    """label vectors [B]: class sizes 1-5 shuffled; all distinct; all equal; one class that holds a whole 32-row tile (B > 32)"""
    g = torch.Generator().manual_seed(seed)
    sizes, n = [], 0
    while n < B:
        k = min(int(torch.randint(1, 6, (1,), generator=g)), B - n)
        sizes.append(k)
        n += k
    mixed = torch.repeat_interleave(torch.arange(len(sizes)) * 7 - 11, torch.tensor(sizes))[torch.randperm(B, generator=g)]
    out = {"mixed": mixed, "distinct": torch.arange(B) - 3, "equal": torch.full((B,), -5)}
    if B > 32:
        t0 = 32 if B >= 64 else 0
        tile = mixed.clone()
        tile[t0:t0 + 32] = 10 ** 12       # (beyond int32: labels are compared as int64)
        out["tile"] = tile
    return out


def device_run(emb, label, kind, p, T, up=UP, grad_scale=1.0):
    o = ops()
    B, D = emb.shape
    e = emb.to(DEV)
    y = label.to(DEV)
    xn, xnT, inv = o.l2norm_fwd(e, T, want_t=True, ldt=(B + 31) // 32 * 32)
    out, stats, ell = o.pair_loss_fwd(xn, y, kind, **p)
    upd = torch.tensor(up, device=DEV)
    dxn = torch.full((B + 1, D), float("nan"), device=DEV)      # a guard row behind the result
    o.pair_loss_bwd(xn, xnT, y, stats, out, kind, grad_scale=grad_scale, grad_scale_dev=upd, dxn=dxn[:B], **p)
    torch.cuda.synchronize()
    assert torch.isnan(dxn[B]).all()
    return dict(xn=xn, xnT=xnT, inv=inv, out=out.cpu(), stats=stats.cpu(), ell=ell.cpu(), dxn=dxn[:B].cpu(), e=e, y=y)


def oracle(xn, label, kind, p, up=UP):
    """float64 on the operand bits -> loss, l, valid, dê * up, W (d loss / d s), q (|d loss / d logit|)"""
    x = xn.cpu().double().requires_grad_(True)
    s = x @ x.t()
    s.retain_grad()
    loss, rows, valid, logits = pair_loss_from_scores(s, label, kind, **p)
    logits.retain_grad()
    loss.backward()
    W = s.grad if s.grad is not None else torch.zeros_like(s)
    q = logits.grad.abs() if logits.grad is not None else torch.zeros_like(s)
    U = W.abs()
    if kind == "supcon" and valid.any():
        # W_ia = (softmax_a - [a in P] / |P|) / (tau A) cancels (to exactly 0 for a lone positive): the rounding of the softmax weight is
        # relative to the weight itself, so the gross magnitude (softmax_a + [a in P] / |P|) / (tau A) carries the relative terms
        B = len(label)
        eye = torch.eye(B, dtype=torch.bool)
        pos = (label[:, None] == label[None, :]) & ~eye
        sm = torch.softmax(logits.detach().masked_fill(eye, float("-inf")), 1) if B > 1 else torch.zeros_like(W)
        U = valid[:, None] * (sm + pos / pos.sum(1).clamp_min(1)[:, None]) / (p["tau"] * valid.sum())
    return dict(loss=loss.item(), rows=rows, valid=valid, dxn=x.grad * up, W=W * up, q=q * up, U=U * abs(up))


def check(r, ref, kind, p, T, B, D, tag):
    delta = D * 2.0 ** -24
    eps = slope_of(kind, p) * delta
    # forward
    assert r["stats"][:, 3].bool().tolist() == ref["valid"].tolist(), tag
    assert r["out"][2].item() == float(ref["valid"].sum()), tag
    fb = 2 * eps
    e_rows = (r["ell"].double() - ref["rows"]).abs().max().item()
    e_loss = abs(r["out"][0].item() - ref["loss"])
    # gradient
    E = (4 * eps + (B + 8) * 2.0 ** -24) * (ref["U"] + ref["U"].t()).sum(1)
    if kind == "circle":
        E = E + p["gamma"] * delta * (ref["q"] + ref["q"].t()).sum(1)
    if T == torch.bfloat16:
        E = E + 2.0 ** -8 * (ref["W"] + ref["W"].t()).abs().sum(1)
    err = (r["dxn"].double() - ref["dxn"]).abs().max(1).values
    live = E > 0
    ratio_g = (err[live] / E[live]).max().item() if live.any() else 0.0
    key = str(T).split(".")[1]
    for what, v in (("rows", e_rows / fb), ("loss", e_loss / fb), ("grad", ratio_g)):
        RATIOS[(kind, what, key)] = max(RATIOS.get((kind, what, key), 0.0), v)
    print(f"{tag}: l_i {e_rows:.3e} loss {e_loss:.3e} (bound {fb:.3e})  grad err/bound {ratio_g:.3f}")
    assert e_rows <= fb and e_loss <= fb, tag
    assert (err <= E).all(), (tag, ratio_g)        # (a row whose bound is 0 must be exactly 0)
    if not ref["valid"].any():
        assert r["out"][0].item() == 0.0 and r["out"][1].item() == 0.0 and (r["dxn"] == 0).all() and (r["ell"] == 0).all(), tag


@pytest.mark.parametrize("D", [8, 40, 512])
@pytest.mark.parametrize("B", [1, 2, 37, 128, 129, 200])
@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_kernels_against_fp64(kind, T, B, D):
    p = KINDS[kind]
    g = torch.Generator().manual_seed(1000 * B + D)
    emb = torch.randn(B, D, generator=g) * (0.5 + 4.0 * torch.rand(B, 1, generator=g))
    for name, label in layouts(B, B + D).items():
        r = device_run(emb, label, kind, p, T)
        ref = oracle(r["xn"], label, kind, p)
        check(r, ref, kind, p, T, B, D, f"{kind} {str(T)[6:]} B={B} D={D} {name}")
    print("largest error / bound so far:", {k: round(v, 4) for k, v in RATIOS.items()})


@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_edge_cases_on_device(kind, T):
    """gamma = 256 / a small temperature, duplicate rows (s = 1), a zero row, a host and a device upstream factor together"""
    B, D = 70, 40
    g = torch.Generator().manual_seed(7)
    emb = torch.randn(B, D, generator=g)
    emb[1] = emb[0]
    emb[40] = emb[0] * 3.0
    emb[5] = 0.0
    label = torch.randint(0, 9, (B,), generator=g)
    label[1] = label[0]
    label[40] = label[0] + 1          # a duplicate among the positives and one among the negatives
    p = dict(m=0.25, gamma=256.0) if kind == "circle" else dict(tau=0.02)
    r = device_run(emb, label, kind, p, T, up=-1.5, grad_scale=2.0)
    assert torch.isfinite(r["out"]).all() and torch.isfinite(r["dxn"]).all() and torch.isfinite(r["ell"]).all()
    assert (r["xn"][5] == 0).all()
    ref = oracle(r["xn"], label, kind, p, up=-3.0)
    check(r, ref, kind, p, T, B, D, f"edge {kind} {str(T)[6:]}")
    # B = 1 and all-distinct labels: no valid anchor -> 0.0 exactly; all-equal labels: circle has no negatives, supcon is valid
    for lab in (torch.arange(B), torch.zeros(B, dtype=torch.long)):
        r = device_run(emb, lab, kind, p, T)
        if kind == "circle" or lab[1] != lab[0]:
            assert r["out"].tolist() == [0.0, 0.0, 0.0] and (r["dxn"] == 0).all() and (r["stats"] == 0).all() and (r["ell"] == 0).all()
        else:
            assert r["out"][2].item() == B and r["out"][0].item() > 0 and torch.isfinite(r["dxn"]).all()


@pytest.mark.parametrize("kind", list(KINDS))
def test_repeatable_bits_and_module_chain(kind):
    """two calls give the same bits (several workgroups: whichever finishes last sums in the same order); the module's loss and embedding
    gradient are the kernel-level results of the same calls, bit for bit"""
    B, D, T = 200, 64, torch.bfloat16
    g = torch.Generator().manual_seed(9)
    emb = torch.randn(B, D, generator=g)
    label = torch.randint(0, 40, (B,), generator=g)
    p = KINDS[kind]
    a = device_run(emb, label, kind, p, T, up=1.0)
    for _ in range(3):
        b = device_run(emb, label, kind, p, T, up=1.0)
        assert torch.equal(a["out"], b["out"]) and torch.equal(a["dxn"], b["dxn"]) and torch.equal(a["ell"], b["ell"])
    e = emb.to(DEV).requires_grad_(True)
    loss = PairLoss(kind, compute_dtype=T, **p)(e, label.to(DEV))
    loss.backward()
    assert loss.shape == () and torch.equal(loss.detach().cpu(), a["out"][0])
    demb = ops().l2norm_bwd(a["e"], a["inv"], a["dxn"].to(DEV), torch.float32)
    assert torch.equal(e.grad, demb)
    # and the whole chain against the CPU module in float64 (normalisation included; bf16 operands: 2^-8 on a score)
    e64 = emb.double().requires_grad_(True)
    ref = pair_loss_torch(e64, label, kind, **p)
    ref.backward()
    assert abs(loss.item() - ref.item()) < 2 * slope_of(kind, p) * 2.0 ** -8
    assert torch.isfinite(e.grad).all() and torch.nn.functional.cosine_similarity(e.grad.cpu().double().flatten(), e64.grad.flatten(), dim=0) > 0.99


class Stem(nn.Module):
    def __init__(self, d_in=24, d=64):
        super().__init__()
        self.fc = nn.Linear(d_in, d)

    def forward(self, x):
        return self.fc(x)


def test_linearity_through_the_module():
    """loss and parameter gradients of SoftmaxBasedMetricLearning(pair_loss=dict(kind='circle', weight=0.5)) = head-only + 0.5 * pair-only,
    within the module-level tolerances of the head tests (1e-4 on the loss, 1e-3 relative on gradients)"""
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    C, B = 20, 16

    def build(**kw):
        torch.manual_seed(3)
        ml = SoftmaxBasedMetricLearning(Stem(), C, 64, is_focal=True, arc_margin=True, **kw)
        ml.add_margin.compute_dtype = torch.float32
        return ml.to(DEV).train()

    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, 24, generator=g).to(DEV)
    y = torch.arange(B).div(4, rounding_mode="floor").to(DEV)          # 4 classes of 4
    both, head = build(pair_loss=dict(kind="circle", weight=0.5)), build()
    ob = both(x, y)
    ob["loss"].backward()
    oh = head(x, y)
    assert set(ob) == set(oh) | {"loss_pair"} and not ob["loss_pair"].requires_grad
    lp = PairLoss("circle", compute_dtype=torch.float32)(oh["emb"], y)
    (oh["loss"] + 0.5 * lp).backward()
    torch.cuda.synchronize()
    assert torch.equal(ob["loss_pair"], lp.detach())
    assert abs(ob["loss"].item() - (oh["loss"].item() + 0.5 * lp.item())) < 1e-4 * max(1.0, abs(ob["loss"].item()))
    for (n, pb), (_, ph) in zip(both.named_parameters(), head.named_parameters()):
        rel = ((pb.grad - ph.grad).norm() / (ph.grad.norm() + 1e-30)).item()
        assert rel < 1e-3, (n, rel)
    # the pair term is really there: without it the embedding layer's gradient differs
    head.zero_grad()
    head(x, y)["loss"].backward()
    assert ((both.module.fc.weight.grad - head.module.fc.weight.grad).norm() / head.module.fc.weight.grad.norm()).item() > 1e-2


def test_centre_free_training_step(tmp_path, monkeypatch, capsys):
    """one PairMetricLearning step through the Controller and the Trainer on the synthetic set with pk = (4, 4); the loss line reports
    loss_pair"""
    import pets_face_recognition_amd as pfr
    from pets_face_recognition_amd.engine import Trainer
    from pets_face_recognition_amd.engine.controller import Controller
    from pets_face_recognition_amd.losses import PairMetricLearning
    pfr.install_reference_aliases()
    monkeypatch.chdir(tmp_path)
    if SYNTH not in sys.path:
        sys.path.insert(0, SYNTH)
    from _common import make
    ns = {}
    make(ns, arch='resnet18', n_train_ids=8, n_val_ids=4, photos=4, image_size=64, train_bs=16, test_bs=8, device='cuda:0',
         limit_train_batches=1, n_pairs=10, compute_dtype=torch.float32, pair_loss=dict(kind='supcon', tau=0.1), pk=(4, 4), centre_free=True)

    class Cfg(dict):
        __getattr__ = dict.get

    torch.manual_seed(11)
    ctrl = Controller(Cfg(ns))
    assert isinstance(ctrl.model_loss, PairMetricLearning)
    batch = next(iter(ns['train_dataloader']()))
    assert sorted(torch.unique(batch['label'], return_counts=True)[1].tolist()) == [4, 4, 4, 4]
    t = Trainer(gpus=[0], max_epochs=1, check_val_every_n_epoch=100, prefetch_batches=0, limit_train_batches=1, log_every_n_steps=1)
    t.fit(ctrl)
    torch.cuda.synchronize()
    assert t.global_step == 1 and len(t.loss_history) == 1 and t.pair_loss_history == t.loss_history
    assert 0 < t.loss_history[0] < 50 and all(torch.isfinite(p).all() for p in ctrl.parameters())
    assert "loss_pair" in capsys.readouterr().out
