"""Cross-batch memory of the pair losses (losses/pair.py) on the CPU: the memory oracle against the batch-only oracle on the concatenation,
finite differences, the ring against a plain deque, the module rules (deferred push, eval / no_grad, warm-up, generation guard, argument
checks) and the C-ABI names."""
import collections
import os

import pytest
import torch

from pets_face_recognition_amd.losses import PairMetricLearning
from pets_face_recognition_amd.losses.pair import (PairLoss, build_pair_loss, pair_loss_from_scores, pair_loss_mem_from_scores,
                                                   pair_loss_mem_torch, pair_loss_torch)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [("supcon", dict(tau=0.1)), ("supcon", dict(tau=0.5)), ("circle", dict(m=0.25, gamma=64.0)), ("circle", dict(m=0.4, gamma=8.0))]


def case(B=9, n=13, D=6, seed=0, shared=True):
    """batch rows (any length), unit memory rows, labels; shared=False: no memory label occurs in the batch"""
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(B, D, generator=g, dtype=torch.float64)
    mem = torch.nn.functional.normalize(torch.randn(n, D, generator=g, dtype=torch.float64), dim=1)
    label = torch.tensor([3, -1, 3, 7, -1, 3, 11, 20, 21][:B])          # 20 and 21 are alone in the batch
    mem_label = torch.randint(0, 4, (n,), generator=g) * 4 - 1 if shared else torch.arange(n) + 100      # {-1, 3, 7, 11} or none
    if shared and n:
        mem_label[0] = 20                                                # an anchor whose only positive is a slot
    return emb, label, mem, mem_label


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "disjoint"])
@pytest.mark.parametrize("kind,params", KINDS)
def test_concatenation_identity(kind, params, shared):
    """l_i of the batch anchors = the first B rows of the batch-only oracle on cat[batch, memory]; the gradient with respect to the batch =
    autograd of sum_{i < B} l_i / A_b on the concatenation with the memory rows detached"""
    emb, label, mem, mem_label = case(shared=shared)
    B = len(label)
    e = emb.clone().requires_grad_(True)
    loss, rows, valid = pair_loss_mem_torch(e, label, mem, mem_label, kind, return_rows=True, **params)
    g, = torch.autograd.grad(loss, e)

    e2 = emb.clone().requires_grad_(True)
    xn = torch.cat([torch.nn.functional.normalize(e2, dim=1, eps=1e-12), mem])
    lab = torch.cat([label, mem_label])
    _, rows_cat, valid_cat = pair_loss_torch(xn.detach(), lab, kind, normalize=False, return_rows=True, **params)
    assert valid.tolist() == valid_cat[:B].tolist()
    assert torch.allclose(rows, rows_cat[:B], rtol=1e-12, atol=1e-12)
    if shared:
        assert valid[7] and not valid[8]             # label 20 is validated by the ring alone, 21 by nothing (supcon) ...
    # the same l_i with a graph: the rows of the concatenation oracle, from its logits
    _, _, _, logits = pair_loss_from_scores(xn @ xn.t(), lab, kind, **params)
    n_all = len(lab)
    eye = torch.eye(n_all, dtype=torch.bool)
    same = lab[:, None] == lab[None, :]
    pos, neg = same & ~eye, ~same
    ninf = float("-inf")
    idx = valid.nonzero().squeeze(1)
    if idx.numel():
        if kind == "supcon":
            ell = torch.logsumexp(logits[idx].masked_fill(eye[idx], ninf), 1) - (logits[idx] * pos[idx]).sum(1) / pos[idx].sum(1)
        else:
            ell = torch.nn.functional.softplus(torch.logsumexp(logits[idx].masked_fill(~neg[idx], ninf), 1)
                                               + torch.logsumexp(logits[idx].masked_fill(~pos[idx], ninf), 1), threshold=1e9)
        ref = ell.sum() / idx.numel()
        # the memory rows are constants of xn (cat of a graph part and a leaf-free tensor): autograd reaches e2 only
        g_ref, = torch.autograd.grad(ref, e2)
        assert abs(loss.item() - ref.item()) < 1e-12 * max(1.0, abs(ref.item()))
        assert torch.allclose(g, g_ref, rtol=1e-10, atol=1e-12)
    else:
        assert loss.item() == 0.0 and torch.equal(g, torch.zeros_like(g))


@pytest.mark.parametrize("kind,params", KINDS)
def test_empty_memory_is_the_batch_loss(kind, params):
    emb, label, mem, mem_label = case()
    a = pair_loss_mem_torch(emb, label, mem[:0], mem_label[:0], kind, return_rows=True, **params)
    b = pair_loss_torch(emb, label, kind, return_rows=True, **params)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    s = torch.nn.functional.normalize(emb, dim=1) @ torch.nn.functional.normalize(emb, dim=1).t()
    x1 = pair_loss_mem_from_scores(s, s[:, :0], label, mem_label[:0], kind, **params)
    x0 = pair_loss_from_scores(s, label, kind, **params)
    assert all(torch.equal(u, v) for u, v in zip(x1, x0))


@pytest.mark.parametrize("kind,params", KINDS)
def test_gradcheck_fp64(kind, params):
    """circle: alpha is a constant in the gradient, so the function differentiated numerically holds it at the evaluation point"""
    emb, label, mem, mem_label = case(seed=1)
    emb.requires_grad_(True)
    fixed = emb.detach().clone()
    f = lambda e: pair_loss_mem_torch(e, label, mem, mem_label, kind, alpha_emb=fixed if kind == "circle" else None, **params)
    assert torch.autograd.gradcheck(f, (emb,), eps=1e-6, atol=1e-6, rtol=1e-5)
    g_plain, = torch.autograd.grad(pair_loss_mem_torch(emb, label, mem, mem_label, kind, **params), emb)
    g_fixed, = torch.autograd.grad(f(emb), emb)
    assert torch.equal(g_plain, g_fixed)
    # nothing flows to the memory
    m = mem.clone().requires_grad_(True)
    pair_loss_mem_torch(emb, label, m, mem_label, kind, **params).backward()
    assert m.grad is None


def test_ring_against_a_deque():
    """B = 37, M = 96, five pushes: the third wraps inside a batch"""
    B, M, D = 37, 96, 8
    pl = PairLoss("supcon", memory=M)
    model = collections.deque(maxlen=M)                 # (row, label) in order of arrival
    slots = {}                                          # slot -> (row, label)
    g = torch.Generator().manual_seed(5)
    head = 0
    for step in range(5):
        xn = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1)
        y = torch.randint(-5, 50, (B,), generator=g)
        pl.push(xn, y)
        for r in range(B):
            model.append((xn[r], int(y[r])))
            slots[(head + r) % M] = (xn[r], int(y[r]))
        head = (head + B) % M
        count = min((step + 1) * B, M)
        assert (pl.head, pl.count, pl.generation) == (head, count, step + 1)
        assert sorted(slots) == list(range(count))                         # the live slots are always 0 .. count - 1
        for k, (row, lab) in slots.items():
            assert torch.equal(pl.mem[k], row) and int(pl.mem_label[k]) == lab
        assert torch.equal(pl.memT[:, :count], pl.mem[:count].t()) and (pl.memT[:, count:] == 0).all()
        # the ring holds exactly the last `count` items
        have = sorted((tuple(pl.mem[k].tolist()), int(pl.mem_label[k])) for k in range(count))
        assert have == sorted((tuple(r.tolist()), l) for r, l in model)
    assert pl.mem.shape == (M, D) and pl.memT.shape == (D, M) and pl.mem_label.dtype == torch.int64
    assert list(pl.state_dict()) == []                                     # not checkpointed
    pl.reset_memory()
    assert pl.mem is None and (pl.head, pl.count) == (0, 0)


def batches(n, B=6, D=5, seed=2):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, D, generator=g, dtype=torch.float64), torch.randint(0, 3, (B,), generator=g)) for _ in range(n)]


@pytest.mark.parametrize("kind", ["supcon", "circle"])
def test_module_push_is_deferred(kind):
    pl = PairLoss(kind, memory=32).train()
    data = batches(3)
    xs = [torch.nn.functional.normalize(e, dim=1, eps=1e-12) for e, _ in data]
    # call 1: an empty ring, nothing pushed yet
    e = data[0][0].clone().requires_grad_(True)
    l1 = pl(e, data[0][1])
    assert (pl.count, pl.generation) == (0, 0) and torch.equal(l1, pair_loss_torch(data[0][0], data[0][1], kind))
    l1.backward()
    # call 2 pushes batch 1 first and pairs with it
    e = data[1][0].clone().requires_grad_(True)
    l2 = pl(e, data[1][1])
    assert (pl.count, pl.head, pl.generation) == (6, 6, 1) and torch.equal(pl.mem[:6], xs[0]) and torch.equal(pl.mem_label[:6], data[0][1])
    ref = pair_loss_mem_torch(data[1][0].clone().requires_grad_(True), data[1][1], xs[0], data[0][1], kind)
    assert torch.equal(l2, ref)
    l2.backward()
    g_ref, = torch.autograd.grad(pair_loss_mem_torch(e, data[1][1], xs[0], data[0][1], kind), e)
    assert torch.equal(e.grad, g_ref)
    # eval mode and no_grad: the ring is read and left alone
    pl.eval()
    le = pl(data[2][0], data[2][1])
    assert (pl.count, pl.generation) == (6, 1) and torch.equal(le, pair_loss_mem_torch(data[2][0], data[2][1], xs[0], data[0][1], kind))
    pl.train()
    with torch.no_grad():
        ln = pl(data[2][0], data[2][1])
    assert (pl.count, pl.generation) == (6, 1) and torch.equal(ln, le)
    # the next training call pushes batch 2 (the last TRAINING call's rows), not the eval batch
    pl(data[2][0].clone().requires_grad_(True), data[2][1])
    assert (pl.count, pl.generation) == (12, 2) and torch.equal(pl.mem[6:12], xs[1])


def test_module_warmup_uses_no_slot_while_the_ring_fills():
    pl = PairLoss("supcon", memory=32, memory_warmup=2).train()
    data = batches(4)
    xs = [torch.nn.functional.normalize(e, dim=1, eps=1e-12) for e, _ in data]
    out = [pl(e.clone().requires_grad_(True), y) for e, y in data[:3]]
    assert pl.count == 12                                                  # two batches pushed by the third call
    assert torch.equal(out[0], pair_loss_torch(*data[0], "supcon")) and torch.equal(out[1], pair_loss_torch(*data[1], "supcon"))
    ref = pair_loss_mem_torch(data[2][0], data[2][1], torch.cat(xs[:2]), torch.cat([data[0][1], data[1][1]]), "supcon")
    assert torch.equal(out[2], ref) and not torch.equal(out[2], pair_loss_torch(*data[2], "supcon"))


def test_module_eval_reads_a_ring_filled_by_hand():
    """push() fills the ring at once; an eval-mode call pairs with it although no training call has happened"""
    pl = PairLoss("supcon", memory=32).eval()
    (e0, y0), (e1, y1) = batches(2)
    x0 = torch.nn.functional.normalize(e0, dim=1, eps=1e-12)
    pl.push(x0, y0)
    out = pl(e1, y1)
    assert torch.equal(out, pair_loss_mem_torch(e1, y1, x0, y0, "supcon")) and not torch.equal(out, pair_loss_torch(e1, y1, "supcon"))
    assert (pl.count, pl.generation, pl.train_calls) == (6, 1, 0)


def test_module_generation_guard():
    pl = PairLoss("circle", memory=32).train()
    data = batches(3)
    l1 = pl(data[0][0].clone().requires_grad_(True), data[0][1])
    l2 = pl(data[1][0].clone().requires_grad_(True), data[1][1])      # pushes batch 1: l1's ring is gone
    with pytest.raises(RuntimeError, match="generation"):
        l1.backward()
    l2.backward()                                                          # the latest forward is fine


def test_module_arguments():
    old = PairLoss("supcon", tau=0.2)
    new = PairLoss("supcon", memory=0, tau=0.2)
    assert list(new.state_dict()) == [] and list(new.buffers()) == [] and repr(new) == repr(old) and new.params == old.params
    e, y = batches(1)[0]
    assert torch.equal(new(e, y), old(e, y)) and torch.equal(new(e, y), pair_loss_torch(e, y, "supcon", tau=0.2))
    with pytest.raises(ValueError, match="takes"):
        PairLoss("supcon", memory=32, gamma=3.0)
    with pytest.raises(ValueError, match="takes"):
        build_pair_loss(dict(kind="circle", memory=32, memory_size=3))
    with pytest.raises(ValueError, match="multiple of 32"):
        PairLoss("supcon", memory=48)
    with pytest.raises(ValueError, match="memory_warmup"):
        PairLoss("supcon", memory_warmup=3)
    with pytest.raises(ValueError, match="larger than the memory"):
        PairLoss("supcon", memory=32)(torch.randn(33, 4), torch.zeros(33, dtype=torch.long))
    pl, w = build_pair_loss(dict(kind="supcon", weight=2.0, memory=64, memory_warmup=1, tau=0.3))
    assert (pl.memory, pl.memory_warmup, w, pl.params) == (64, 1, 2.0, dict(tau=0.3))
    # a later change of D (or dtype) is an error
    pl.train()
    pl(torch.randn(4, 8), torch.zeros(4, dtype=torch.long))
    pl(torch.randn(4, 8), torch.zeros(4, dtype=torch.long))
    with pytest.raises(ValueError, match="rows of length"):
        pl(torch.randn(4, 16), torch.zeros(4, dtype=torch.long))
    with pytest.raises(ValueError, match="rows of length"):
        pl(torch.randn(4, 8, dtype=torch.float64), torch.zeros(4, dtype=torch.long))
    ml = PairMetricLearning(torch.nn.Linear(5, 8), dict(kind="supcon", memory=32), embedding_size=8)
    assert ml.pair_loss.memory == 32 and list(ml.state_dict()) == ["module.weight", "module.bias"]


def test_thunks_and_header_name_the_entry_points():
    from pets_face_recognition_amd._hip.lib import parse_header
    protos = parse_header()
    inc = open(os.path.join(ROOT, "pets-face-recognition_amd", "csrc", "pfr_thunks_gen.inc")).read()
    for name, nargs in (("pfr_pair_mem_loss_fwd", 19), ("pfr_pair_mem_loss_bwd", 24), ("pfr_pair_mem_push", 12)):
        assert name in protos and len(protos[name][1]) == nargs
        assert f'{{"{name}", th_{name}}}' in inc
    assert "pfr_pair_mem_splits" in protos and "th_pfr_pair_mem_splits" not in inc      # host arithmetic: no stream, no thunk
