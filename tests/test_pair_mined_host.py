"""The mined pair losses (batch-hard triplet, Multi-Similarity) on the CPU: the torch form of the contract (losses/pair.py:
pair_mined_parts behind pair_loss_from_scores / pair_loss_mem_from_scores) against a naive per-anchor Python loop, the constant-in-gradient
mining by central finite differences, the tie rule, the parameter checks, the module plumbing and the C-ABI argument errors."""
import ctypes
import math
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from pets_face_recognition_amd.losses import PairMetricLearning
from pets_face_recognition_amd.losses.pair import (KINDS, PairLoss, build_pair_loss, pair_loss_from_scores, pair_loss_mem_from_scores,
                                                   pair_loss_mem_torch, pair_loss_torch, pair_mined_parts)

MINED = [("batch_hard", dict(m=0.3, gamma=0.0)), ("batch_hard", dict(m=0.1, gamma=4.0)),
         ("multi_similarity", dict(alpha=2.0, beta=50.0, base=0.5, epsilon=0.1)), ("multi_similarity", dict(alpha=1.5, beta=8.0, base=0.25, epsilon=0.02))]


def naive(sb, sm, label, mlabel, kind, p):
    """per-anchor loop over python floats -> loss, rows, valid, ip, in, kept (partner number j for batch item j, B + k for slot k)"""
    B, n = len(label), len(label) + len(mlabel)
    lab = list(label) + list(mlabel)
    rows, valid, ips, ins, kept = [], [], [], [], []
    for i in range(B):
        sc = [float(v) for v in sb[i]] + [float(v) for v in sm[i]]
        P = [j for j in range(n) if j != i and lab[j] == label[i] and not math.isnan(sc[j])]
        N = [j for j in range(n) if lab[j] != label[i] and not math.isnan(sc[j])]
        if not P or not N:
            rows.append(0.0); valid.append(False); ips.append(-1); ins.append(-1); kept.append(0)
            continue
        ip = min(P, key=lambda j: (sc[j], j))
        inn = min(N, key=lambda j: (-sc[j], j))
        if kind == "batch_hard":
            z = sc[inn] - sc[ip] + p["m"]
            g = p["gamma"]
            l = max(0.0, z) if g == 0 else (max(g * z, 0.0) + math.log1p(math.exp(-abs(g * z)))) / g
            k = 2
        else:
            kp = [j for j in P if sc[j] - p["epsilon"] < sc[inn]]
            kn = [j for j in N if sc[j] + p["epsilon"] > sc[ip]]
            l = math.log(1 + sum(math.exp(-p["alpha"] * (sc[j] - p["base"])) for j in kp)) / p["alpha"] \
                + math.log(1 + sum(math.exp(p["beta"] * (sc[j] - p["base"])) for j in kn)) / p["beta"]
            k = len(kp) + len(kn)
        rows.append(l); valid.append(True); ips.append(ip); ins.append(inn); kept.append(k)
    A = sum(valid)
    return (sum(rows) / A if A else 0.0), rows, valid, ips, ins, kept


def parts_of(xn, label, mem, mlabel, kind, p):
    B, n = xn.shape[0], mem.shape[0]
    s = torch.cat([xn @ xn.t(), xn @ mem.t()], 1)
    same = label[:, None] == torch.cat([label, mlabel])[None, :]
    eye = torch.cat([torch.eye(B, dtype=torch.bool), torch.zeros(B, n, dtype=torch.bool)], 1)
    return pair_mined_parts(s, same & ~eye, ~same, kind, **p)


LAYOUTS = {
    "mixed": ([0, 1, 1, 2, 0, 2, 2, 5, 1], [1, 7, 0, 0, 9]),
    "distinct": (list(range(7)), [20, 21, 22]),
    "equal": ([4] * 6, [4, 4]),
    "one": ([3], [3, 8, 3]),
    "ring_only_positive": ([0, 1, 2, 3], [0, 1, 9, 9]),          # every positive of an anchor lives in the ring
}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("with_mem", [False, True], ids=["batch", "ring"])
@pytest.mark.parametrize("kind,p", MINED)
def test_oracle_against_the_naive_loop(kind, p, with_mem, layout):
    lab, mlab = LAYOUTS[layout]
    D = 6
    g = torch.Generator().manual_seed(len(lab) * 7 + len(mlab))
    emb = torch.randn(len(lab), D, generator=g, dtype=torch.float64).requires_grad_(True)
    mem = F.normalize(torch.randn(len(mlab), D, generator=g, dtype=torch.float64), dim=1)
    label, mlabel = torch.tensor(lab), torch.tensor(mlab)
    if not with_mem:
        mem, mlabel, mlab = mem[:0], mlabel[:0], []            # also: an empty ring through the memory form
        loss_b, rows_b, valid_b = pair_loss_torch(emb, label, kind, return_rows=True, **p)
    loss, rows, valid = pair_loss_mem_torch(emb, label, mem, mlabel, kind, return_rows=True, **p)
    xn = F.normalize(emb.detach(), dim=1)
    ref = naive(xn @ xn.t(), xn @ mem.t(), lab, mlab, kind, p)
    assert valid.tolist() == ref[2]
    assert torch.allclose(rows, torch.tensor(ref[1], dtype=torch.float64), rtol=1e-12, atol=1e-13)
    assert abs(loss.item() - ref[0]) < 1e-12
    r = parts_of(xn, label, mem, mlabel, kind, p)
    assert r["ip"].tolist() == ref[3] and r["inn"].tolist() == ref[4] and r["keep"].sum(1).tolist() == ref[5]
    if not with_mem:
        assert torch.equal(loss_b, loss) and torch.equal(rows_b, rows) and torch.equal(valid_b, valid)
    gr, = torch.autograd.grad(loss, emb)
    if not any(ref[2]):                                           # A = 0: exactly 0.0 and a zero gradient
        assert loss.item() == 0.0 and (gr == 0).all() and (rows == 0).all()
    else:
        assert torch.isfinite(gr).all()
    if layout == "ring_only_positive":
        assert valid.tolist() == ([True, True, False, False] if with_mem else [False] * 4)


def boundary_margin(xn, label, mem, mlabel, kind, p):
    """the smallest distance of any score (or z_i) to a decision boundary: two candidates for an extreme against each other, a pair
    against its mining threshold, z_i against 0"""
    r = parts_of(xn, label, mem, mlabel, kind, p)
    B, n = xn.shape[0], xn.shape[0] + mem.shape[0]
    s = torch.cat([xn @ xn.t(), xn @ mem.t()], 1)
    same = label[:, None] == torch.cat([label, mlabel])[None, :]
    eye = torch.cat([torch.eye(B, dtype=torch.bool), torch.zeros(B, n - B, dtype=torch.bool)], 1)
    pos, neg = same & ~eye, ~same
    gaps = []
    for i in range(B):
        if not r["valid"][i]:
            continue
        sp, sn = r["sp"][i], r["sn"][i]
        others_p = pos[i].clone(); others_p[r["ip"][i]] = False
        others_n = neg[i].clone(); others_n[r["inn"][i]] = False
        if others_p.any():
            gaps.append((s[i][others_p] - sp).min().item())
        if others_n.any():
            gaps.append((sn - s[i][others_n]).min().item())
        if kind == "batch_hard":
            if p["gamma"] == 0:
                gaps.append(abs(r["a"][i].item()))
        else:
            gaps.append((s[i][neg[i]] + p["epsilon"] - sp).abs().min().item())
            gaps.append((s[i][pos[i]] - p["epsilon"] - sn).abs().min().item())
    return min(gaps)


@pytest.mark.parametrize("with_mem", [False, True], ids=["batch", "ring"])
@pytest.mark.parametrize("kind,p", MINED)
def test_mining_is_a_constant_in_the_gradient(kind, p, with_mem):
    """central finite differences of the whole loss (selection recomputed at every point) equal autograd, in which the selection is a
    constant: true as long as no decision changes inside the step, which the margin assertion guarantees first"""
    h = 1e-6
    lab, mlab = [0, 1, 1, 2, 0, 2, 2], [1, 0, 5]
    g = torch.Generator().manual_seed(3)
    emb = torch.randn(len(lab), 5, generator=g, dtype=torch.float64)
    emb = emb / emb.norm(dim=1, keepdim=True) * 1.5                 # |e| = 1.5: a step h moves a score by less than h
    mem = F.normalize(torch.randn(len(mlab), 5, generator=g, dtype=torch.float64), dim=1)
    label, mlabel = torch.tensor(lab), torch.tensor(mlab)
    if not with_mem:
        mem, mlabel = mem[:0], mlabel[:0]
    assert boundary_margin(F.normalize(emb, dim=1), label, mem, mlabel, kind, p) >= 100 * h

    def f(e):
        return pair_loss_mem_torch(e, label, mem, mlabel, kind, **p)

    e = emb.clone().requires_grad_(True)
    loss = f(e)
    assert loss.item() > 0
    gr, = torch.autograd.grad(loss, e)
    fd = torch.zeros_like(emb)
    for i in range(emb.shape[0]):
        for d in range(emb.shape[1]):
            ep, em = emb.clone(), emb.clone()
            ep[i, d] += h
            em[i, d] -= h
            fd[i, d] = (f(ep) - f(em)) / (2 * h)
    assert torch.allclose(gr, fd, rtol=1e-6, atol=1e-8), (gr - fd).abs().max()
    assert gr.abs().sum() > 0


def test_tie_rule_smallest_partner_number_and_batch_before_ring():
    # anchor 0 (label 0): positives at the partner numbers 2, 3 (batch) and 5 (slot 1), negatives 1 (batch), 4 and 6 (slots 0, 2)
    label, mlabel = torch.tensor([0, 1, 0, 0]), torch.tensor([1, 0, 1])
    sb = torch.tensor([[1.0, 0.5, 0.25, 0.25], [0.5, 1.0, 0.0, 0.0], [0.25, 0.0, 1.0, -0.0], [0.25, 0.0, 0.0, 1.0]], dtype=torch.float64)
    sm = torch.tensor([[0.5, 0.25, 0.5], [0.0, -0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    s = torch.cat([sb, sm], 1)
    same = label[:, None] == torch.cat([label, mlabel])[None, :]
    eye = torch.cat([torch.eye(4, dtype=torch.bool), torch.zeros(4, 3, dtype=torch.bool)], 1)
    for kind in ("batch_hard", "multi_similarity"):
        r = pair_mined_parts(s, same & ~eye, ~same, kind)
        assert (r["ip"][0].item(), r["inn"][0].item()) == (2, 1)            # 2 before 3 before slot 1 (= 5); batch item 1 before slot 0 (= 4)
        assert (r["sp"][0].item(), r["sn"][0].item()) == (0.25, 0.5)
        # anchor 1 (label 1): positives are the slots 0 and 2 (numbers 4, 6) at 0.0; negatives 0, 2, 3 and slot 1 (-0.0 ties with +0.0)
        assert (r["ip"][1].item(), r["inn"][1].item()) == (4, 0)
        # anchor 2: positives 0 (0.25), 3 (-0.0), slot 1 (0.0): -0.0 = +0.0, so number 3 wins over number 5
        assert r["ip"][2].item() == 3
    # with the ring slot alone holding the minimum, the slot wins
    s2 = s.clone()
    s2[0, 5] = 0.125
    assert pair_mined_parts(s2, same & ~eye, ~same, "batch_hard")["ip"][0].item() == 5
    # a NaN score is in neither set
    s3 = s.clone()
    s3[0, 2] = float("nan")
    r = pair_mined_parts(s3, same & ~eye, ~same, "batch_hard")
    assert r["ip"][0].item() == 3 and torch.isfinite(r["rows"]).all()


def test_hinge_is_inactive_at_zero():
    """z_i = 0 exactly: l_i = 0 and NO gradient (active iff z_i > 0), as the device kernel has it"""
    s = torch.tensor([[1.0, 0.5, 0.25, 0.0], [0.5, 1.0, 0.0, 0.25], [0.25, 0.0, 1.0, 0.25], [0.0, 0.25, 0.25, 1.0]], dtype=torch.float64,
                     requires_grad=True)
    label = torch.tensor([0, 0, 1, 1])
    loss, rows, valid, _ = pair_loss_from_scores(s, label, "batch_hard", m=0.25, gamma=0.0)      # anchors 0, 1: z = 0.25 - 0.5 + 0.25 = 0
    gr, = torch.autograd.grad(loss, s)
    assert valid.all() and rows.tolist() == [0.0, 0.0, 0.25, 0.25] and loss.item() == 0.125
    assert (gr[:2] == 0).all() and gr[2].tolist() == [0.25, 0.0, 0.0, -0.25] and gr[3].tolist() == [0.0, 0.25, -0.25, 0.0]


def test_multi_similarity_with_everything_kept_is_the_unmined_formula():
    g = torch.Generator().manual_seed(8)
    B = 9
    emb = torch.randn(B, 6, generator=g, dtype=torch.float64)
    label = torch.tensor([0, 1, 1, 2, 0, 2, 2, 5, 1])
    al, be, lam = 2.0, 10.0, 0.5
    loss, rows, valid = pair_loss_torch(emb, label, "multi_similarity", return_rows=True, alpha=al, beta=be, base=lam, epsilon=4.0)
    xn = F.normalize(emb, dim=1)
    s = xn @ xn.t()
    same = label[:, None] == label[None, :]
    pos, neg = same & ~torch.eye(B, dtype=torch.bool), ~same
    ref = torch.log1p((torch.exp(-al * (s - lam)) * pos).sum(1)) / al + torch.log1p((torch.exp(be * (s - lam)) * neg).sum(1)) / be
    assert valid.tolist() == (pos.any(1) & neg.any(1)).tolist() and not valid.all()
    assert torch.allclose(rows[valid], ref[valid], rtol=1e-12) and abs(loss.item() - ref[valid].mean().item()) < 1e-12


def test_large_beta_stays_finite():
    g = torch.Generator().manual_seed(9)
    emb = torch.randn(12, 8, generator=g)
    label = torch.arange(12) % 4
    for dt in (torch.float32, torch.float64):
        e = emb.to(dt).requires_grad_(True)
        loss = pair_loss_torch(e, label, "multi_similarity", beta=256.0, alpha=64.0)
        gr, = torch.autograd.grad(loss, e)
        assert torch.isfinite(loss) and torch.isfinite(gr).all() and loss.item() > 0


def test_bad_parameters():
    assert KINDS == ("supcon", "circle", "batch_hard", "multi_similarity")
    with pytest.raises(ValueError, match="kind"):
        PairLoss("triplet")
    with pytest.raises(ValueError, match="takes"):
        PairLoss("batch_hard", tau=0.1)
    with pytest.raises(ValueError, match="takes"):
        PairLoss("multi_similarity", m=0.1)
    with pytest.raises(ValueError, match="margin"):
        PairLoss("batch_hard", m=-0.1)
    with pytest.raises(ValueError, match="gamma"):
        PairLoss("batch_hard", gamma=-1.0)
    for bad in (dict(alpha=0.0), dict(beta=-1.0), dict(epsilon=-0.1), dict(base=float("nan"))):
        with pytest.raises(ValueError, match="multi_similarity"):
            PairLoss("multi_similarity", **bad)
    assert PairLoss("batch_hard").params == dict(m=0.3, gamma=0.0)
    assert PairLoss("multi_similarity").params == dict(alpha=2.0, beta=50.0, base=0.5, epsilon=0.1)
    assert "kind='multi_similarity', alpha=2, beta=50, base=0.5, epsilon=0.1" in repr(PairLoss("multi_similarity"))
    mod, w = build_pair_loss(dict(kind="batch_hard", weight=0.5, m=0.2, memory=64))
    assert w == 0.5 and mod.kind == "batch_hard" and mod.memory == 64 and mod.params["m"] == 0.2
    from pets_face_recognition_amd._hip import ops
    with pytest.raises(ValueError, match="kind"):
        ops.pair_mined_params("circle")
    k, p4 = ops.pair_mined_params("multi_similarity", beta=8.0)
    assert k == 3 and list(p4) == [2.0, 8.0, 0.5, pytest.approx(0.1)]
    assert ops.pair_mined_params("batch_hard")[0] == 2


class Stem(nn.Module):
    def __init__(self, d_in=12, d=16):
        super().__init__()
        self.fc = nn.Linear(d_in, d)

    def forward(self, x):
        return self.fc(x)


@pytest.mark.parametrize("memory", [0, 32])
@pytest.mark.parametrize("kind", ["batch_hard", "multi_similarity"])
def test_pair_metric_learning_builds_with_the_mined_kinds(kind, memory):
    torch.manual_seed(5)
    ml = PairMetricLearning(Stem(), dict(kind=kind, weight=2.0, memory=memory), embedding_size=16)
    x = torch.randn(6, 12)
    y = torch.tensor([0, 1, 1, 4, 0, 2])
    out = ml(x, y)
    assert set(out) == {"loss", "emb", "logits", "loss_pair"} and out["logits"] is None
    ref = pair_loss_torch(ml(x), y, kind)
    assert torch.allclose(out["loss_pair"], ref) and torch.allclose(out["loss"], 2.0 * ref) and ref.item() > 0
    out["loss"].backward()
    assert ml.module.fc.weight.grad.abs().sum() > 0
    if memory:                                                      # the deferred push: the second call pairs with the first batch
        ring = ml.pair_loss
        assert ring.count == 0 and ring._pending is not None
        out2 = ml(x, y)
        assert (ring.count, ring.generation) == (6, 1)
        ref2 = pair_loss_mem_torch(ml(x), y, ring.mem[:6], ring.mem_label[:6], kind)
        assert torch.allclose(out2["loss_pair"], ref2)
        ml(x, y)                                                    # a third forward pushes before out2's backward has run
        with pytest.raises(RuntimeError, match="generation"):
            out2["loss"].backward()


# ------------------------------------------------------------------------------------------------ C-ABI
def test_abi_exports_the_mined_kernels():
    from pets_face_recognition_amd._hip.lib import LIB_PATH, parse_header
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    protos = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    for name, nargs in (("pfr_pair_mined_fwd", 18), ("pfr_pair_mined_bwd", 23), ("pfr_pair_mined_splits", 3)):
        assert name in protos and len(protos[name][1]) == nargs
        assert hasattr(dll, name)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    thunks = open(os.path.join(root, "pets-face-recognition_amd", "csrc", "pfr_thunks_gen.inc")).read()
    assert "th_pfr_pair_mined_fwd" in thunks and "th_pfr_pair_mined_bwd" in thunks


def test_abi_argument_errors():
    from pets_face_recognition_amd._hip import lib, ops, PfrError
    p4 = (ctypes.c_float * 4)(2.0, 50.0, 0.5, 0.1)
    with pytest.raises(PfrError, match="null pointer"):
        lib.pfr_pair_mined_fwd(0, 0, 0, 4, 8, 0, 0, 0, 0, 3, p4, 0, 0, 0, 0, 0, 0, 0)
    with pytest.raises(PfrError, match="null pointer"):
        lib.pfr_pair_mined_fwd(16, 0, 16, 4, 8, 0, 0, 0, 0, 3, 0, 0, 0, 16, 16, 16, 16, 0)
    with pytest.raises(PfrError, match="int8 is not supported"):
        lib.pfr_pair_mined_fwd(16, 2, 16, 4, 8, 0, 0, 0, 0, 3, p4, 0, 0, 16, 16, 16, 16, 0)
    with pytest.raises(PfrError, match="multiple of 8"):
        lib.pfr_pair_mined_fwd(16, 0, 16, 4, 12, 0, 0, 0, 0, 3, p4, 0, 0, 16, 16, 16, 16, 0)
    with pytest.raises(PfrError, match="kind must be 2"):
        lib.pfr_pair_mined_fwd(16, 0, 16, 4, 8, 0, 0, 0, 0, 1, p4, 0, 0, 16, 16, 16, 16, 0)
    with pytest.raises(PfrError, match="alpha > 0"):
        lib.pfr_pair_mined_fwd(16, 0, 16, 4, 8, 0, 0, 0, 0, 3, (ctypes.c_float * 4)(0.0, 50.0, 0.5, 0.1), 0, 0, 16, 16, 16, 16, 0)
    with pytest.raises(PfrError, match="margin >= 0"):
        lib.pfr_pair_mined_fwd(16, 0, 16, 4, 8, 0, 0, 0, 0, 2, (ctypes.c_float * 4)(-1.0, 0.0, 0.0, 0.0), 0, 0, 16, 16, 16, 16, 0)
    with pytest.raises(PfrError, match="without a ring"):
        lib.pfr_pair_mined_fwd(16, 0, 16, 4, 8, 0, 0, 32, 0, 3, p4, 0, 0, 16, 16, 16, 16, 0)
    with pytest.raises(PfrError, match="the ring needs M"):
        lib.pfr_pair_mined_fwd(16, 0, 16, 4, 8, 16, 16, 33, 0, 3, p4, 0, 0, 16, 16, 16, 16, 0)
    with pytest.raises(PfrError, match="workspace required"):
        lib.pfr_pair_mined_fwd(16, 0, 16, 4, 8, 0, 0, 0, 0, 3, p4, 2, 0, 16, 16, 16, 16, 0)
    with pytest.raises(PfrError, match="ldt"):
        lib.pfr_pair_mined_bwd(16, 16, 0, 40, 16, 33, 8, 0, 0, 0, 0, 0, 0, 3, p4, 16, 16, 1.0, 0, 1, 0, 16, 0)
    assert lib.pfr_pair_mined_splits(256, 65536, 512) == lib.pfr_pair_mem_splits(256, 65536, 512) == 32
    with pytest.raises(PfrError, match="no CPU fallback"):
        ops.pair_mined_fwd(torch.zeros(4, 8), torch.zeros(4, dtype=torch.long), "batch_hard")
