"""Pair losses with a cross-batch memory on the device (csrc/pfr_pairmem.hip) against the float64 CPU implementation of the contract
(losses/pair.py: pair_loss_mem_from_scores), by the scheme of tests/test_pair_loss_gpu.py: the oracle is evaluated in float64 ON THE
OPERAND BITS (ê as pfr_l2norm_fwd wrote it, the ring rows as they are stored), every l_i, the scalar, A, the validity flags and every
component of dê are compared, the upstream gradient is a device scalar != 1, a NaN guard row stands behind dê, and the slots >= count of
the ring are NaN.

Bounds (derived, not tuned; observed / bound is printed and the largest ratios are recorded in profiles/pair_memory.txt).  With n = B +
count partners and S partner-range splits:
  delta = D * 2^-24, eps = slope * delta as in tests/test_pair_loss_gpu.py.
  merge     the S partial (max, sum) states of an anchor are merged one after the other: each merge scales a sum by an expf (<= 2 ulp =
            4 * 2^-24 relative) and adds (one multiply, one add: 2 * 2^-24), so a log-sum-exp moves by <= 6 S 2^-24 absolutely, and l_i,
            which holds two of them for circle, by mu = 12 S 2^-24.
  forward   |d l_i| <= 2 eps + mu; the scalar is a mean of l_i: the same bound.
  gradient  the batch file's row bound with: the summation term over n partners instead of B; the statistics of an anchor shifted by the
            merges (a softmax weight and sigma(z) move by mu relatively); the S slabs summed one after the other (S * 2^-24 relative to
            sum |G|); and the W^T parts restricted to the batch partners, because a slot is never an anchor:
              E_r = (4 eps + mu + (n + 8 + S) 2^-24) (sum_{j in batch} (U_rj + U_jr) + sum_k U_rk)
                    + gamma delta (sum_{j in batch} (q_rj + q_jr) + sum_k q_rk)
              bf16: + 2^-8 (sum_{j in batch} |W_rj + W_jr| + sum_k |W_rk|)
            all times the upstream gradient.
The partner tiles are ceil(B / 32) batch tiles followed by ceil(count / 32) memory tiles: B = 37, count = 100 is 2 + 4 = 6 tiles, so
splits = 7 has an empty split."""
import os
import sys

import pytest
import torch

from pets_face_recognition_amd.losses.pair import PairLoss, pair_loss_mem_from_scores, pair_loss_mem_torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTH = os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic")
KINDS = {"supcon": dict(tau=0.1), "circle": dict(m=0.25, gamma=64.0)}
DTYPES = [torch.float32, torch.bfloat16]
RINGS = [(32, 0), (32, 1), (32, 32), (128, 31), (128, 33), (128, 100), (128, 128)]
UP = 0.75
RATIOS = {}


def ops():
    from pets_face_recognition_amd._hip import ops as o
    return o


def slope_of(kind, p):
    return 1.0 / p["tau"] if kind == "supcon" else p["gamma"] * (1.0 + p["m"])


def layouts(B, seed):
    """label vectors [B] as in tests/test_pair_loss_gpu.py: class sizes 1-5 shuffled; all distinct; one class over a whole tile (B > 32)"""
    g = torch.Generator().manual_seed(seed)
    sizes, n = [], 0
    while n < B:
        k = min(int(torch.randint(1, 6, (1,), generator=g)), B - n)
        sizes.append(k)
        n += k
    mixed = torch.repeat_interleave(torch.arange(len(sizes)) * 7 - 11, torch.tensor(sizes))[torch.randperm(B, generator=g)]
    out = {"mixed": mixed, "distinct": torch.arange(B) - 3}
    if B > 32:
        t0 = 32 if B >= 64 else 0
        tile = mixed.clone()
        tile[t0:t0 + 32] = 10 ** 12
        out["tile"] = tile
    return out


def make_ring(M, count, D, T, seed, rows=None):
    """mem [M, D] with NaN at the slots >= count, memT [D, M] zero there; the live rows are l2norm_fwd's output for random rows"""
    g = torch.Generator().manual_seed(seed)
    mem = torch.full((M, D), float("nan"), dtype=T, device=DEV)
    memT = torch.zeros((D, M), dtype=T, device=DEV)
    if count:
        live = ops().l2norm_fwd((torch.randn(count, D, generator=g) * 3).to(DEV), T)[0] if rows is None else rows
        mem[:count] = live
        memT[:, :count] = live.t()
    return mem, memT


def device_run(emb, label, mem, memT, mem_label, count, kind, p, T, up=UP, grad_scale=1.0, splits=0):
    o = ops()
    B, D = emb.shape
    e, y = emb.to(DEV), label.to(DEV)
    xn, xnT, inv = o.l2norm_fwd(e, T, want_t=True, ldt=(B + 31) // 32 * 32)
    out, stats, ell = o.pair_mem_loss_fwd(xn, y, mem, mem_label, count, kind, splits=splits, **p)
    upd = torch.tensor(up, device=DEV)
    dxn = torch.full((B + 1, D), float("nan"), device=DEV)
    o.pair_mem_loss_bwd(xn, xnT, y, mem, memT, mem_label, count, stats, out, kind, grad_scale=grad_scale, grad_scale_dev=upd, dxn=dxn[:B],
                        splits=splits, **p)
    torch.cuda.synchronize()
    assert torch.isnan(dxn[B]).all()
    return dict(xn=xn, xnT=xnT, inv=inv, out=out.cpu(), stats=stats.cpu(), ell=ell.cpu(), dxn=dxn[:B].cpu(), e=e, y=y)


def oracle(xn, label, mem, mem_label, count, kind, p, up=UP):
    """float64 on the operand bits -> loss, l, valid, dê * up, W = d loss / d s [B, B + count], q = |d loss / d logit|, U"""
    x = xn.cpu().double().requires_grad_(True)
    m = mem[:count].cpu().double()
    ml = mem_label[:count].cpu()
    B = len(label)
    sb, sm = x @ x.t(), x @ m.t()
    sb.retain_grad(); sm.retain_grad()
    loss, rows, valid, logits = pair_loss_mem_from_scores(sb, sm, label, ml, kind, **p)
    logits.retain_grad()
    loss.backward()
    zb, zm = torch.zeros(B, B, dtype=torch.float64), torch.zeros(B, count, dtype=torch.float64)
    W = torch.cat([sb.grad if sb.grad is not None else zb, sm.grad if sm.grad is not None else zm], 1)
    q = logits.grad.abs() if logits.grad is not None else torch.zeros_like(W)
    U = W.abs()
    if kind == "supcon" and valid.any():
        eye = torch.cat([torch.eye(B, dtype=torch.bool), torch.zeros(B, count, dtype=torch.bool)], 1)
        pos = (label[:, None] == torch.cat([label, ml])[None, :]) & ~eye
        soft = torch.softmax(logits.detach().masked_fill(eye, float("-inf")), 1) if B + count > 1 else torch.zeros_like(W)
        U = valid[:, None] * (soft + pos / pos.sum(1).clamp_min(1)[:, None]) / (p["tau"] * valid.sum())
    dx = x.grad if x.grad is not None else torch.zeros_like(x)
    return dict(loss=loss.item(), rows=rows, valid=valid, dxn=dx * up, W=W * up, q=q * up, U=U * abs(up))


def sym(X, B):
    """row sums of the bound: (X + X^T) over the batch partners, X alone over the slots"""
    return (X[:, :B] + X[:, :B].t()).sum(1) + X[:, B:].sum(1)


def check(r, ref, kind, p, T, B, D, count, S, tag):
    delta = D * 2.0 ** -24
    eps = slope_of(kind, p) * delta
    mu = 12 * S * 2.0 ** -24
    assert r["stats"][:, 3].bool().tolist() == ref["valid"].tolist(), tag
    assert r["out"][2].item() == float(ref["valid"].sum()), tag
    fb = 2 * eps + mu
    e_rows = (r["ell"].double() - ref["rows"]).abs().max().item()
    e_loss = abs(r["out"][0].item() - ref["loss"])
    E = (4 * eps + mu + (B + count + 8 + S) * 2.0 ** -24) * sym(ref["U"], B)
    if kind == "circle":
        E = E + p["gamma"] * delta * sym(ref["q"], B)
    if T == torch.bfloat16:
        W = ref["W"]
        E = E + 2.0 ** -8 * ((W[:, :B] + W[:, :B].t()).abs().sum(1) + W[:, B:].abs().sum(1))
    err = (r["dxn"].double() - ref["dxn"]).abs().max(1).values
    live = E > 0
    ratio_g = (err[live] / E[live]).max().item() if live.any() else 0.0
    key = str(T).split(".")[1]
    for what, v in (("rows", e_rows / fb), ("loss", e_loss / fb), ("grad", ratio_g)):
        RATIOS[(kind, what, key)] = max(RATIOS.get((kind, what, key), 0.0), v)
    print(f"{tag}: l_i {e_rows:.3e} loss {e_loss:.3e} (bound {fb:.3e})  grad err/bound {ratio_g:.3f}")
    assert torch.isfinite(r["out"]).all() and torch.isfinite(r["ell"]).all() and torch.isfinite(r["dxn"]).all() and torch.isfinite(r["stats"]).all(), tag
    assert e_rows <= fb and e_loss <= fb, tag
    assert (err <= E).all(), (tag, ratio_g)        # (a row whose bound is 0 must be exactly 0)
    if not ref["valid"].any():
        assert r["out"][0].item() == 0.0 and r["out"][1].item() == 0.0 and (r["dxn"] == 0).all() and (r["ell"] == 0).all(), tag


def mem_labels(label, M, how, seed):
    """'shared': drawn from the batch's label values (garbage slots too, so that a slot >= count would count if it were read);
    'disjoint': no label of the batch"""
    g = torch.Generator().manual_seed(seed)
    if how == "shared":
        return label[torch.randint(0, len(label), (M,), generator=g)].to(DEV)
    return (torch.arange(M) + 10 ** 6).to(DEV)


def run_case(kind, T, B, D, M, count, splits=0):
    p = KINDS[kind]
    g = torch.Generator().manual_seed(1000 * B + D + count)
    emb = torch.randn(B, D, generator=g) * (0.5 + 4.0 * torch.rand(B, 1, generator=g))
    mem, memT = make_ring(M, count, D, T, B + count)
    S = splits or ops().pair_mem_splits(B, count, D)
    for name, label in layouts(B, B + D).items():
        for how in ("shared", "disjoint"):
            ml = mem_labels(label, M, how, count)
            r = device_run(emb, label, mem, memT, ml, count, kind, p, T, splits=splits)
            ref = oracle(r["xn"], label, mem, ml, count, kind, p)
            check(r, ref, kind, p, T, B, D, count, S, f"{kind} {str(T)[6:]} B={B} D={D} M={M} count={count} S={S} {name}/{how}")


@pytest.mark.parametrize("D", [8, 40])
@pytest.mark.parametrize("T", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_kernels_against_fp64(kind, T, D):
    for B in (1, 37, 70):
        for M, count in RINGS:
            run_case(kind, T, B, D, M, count)
    print("largest error / bound so far:", {k: round(v, 4) for k, v in RATIOS.items()})


@pytest.mark.parametrize("T", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_kernels_against_fp64_d512(kind, T):
    run_case(kind, T, 37, 512, 128, 100)
    print("largest error / bound so far:", {k: round(v, 4) for k, v in RATIOS.items()})


@pytest.mark.parametrize("T", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_split_handling(kind, T):
    """B = 37, count = 100: 2 + 4 tiles; 1, 2, 3 and 7 splits (7: an empty split) are within the bounds and bit-identical over four calls;
    splits = 0 is pair_mem_splits"""
    B, D, M, count = 37, 40, 128, 100
    p = KINDS[kind]
    g = torch.Generator().manual_seed(21)
    emb = torch.randn(B, D, generator=g)
    label = layouts(B, 3)["mixed"]
    mem, memT = make_ring(M, count, D, T, 22)
    ml = mem_labels(label, M, "shared", 23)
    auto = ops().pair_mem_splits(B, count, D)
    assert auto == 2                                    # min(256 / 2 anchor blocks, ceil(6 tiles / 4), budget)
    assert ops().pair_mem_splits(256, 65536, 512) == 32 and ops().pair_mem_splits(1, 0, 8) == 1
    res = {}
    for S in (0, 1, 2, 3, 7):
        a = device_run(emb, label, mem, memT, ml, count, kind, p, T, splits=S)
        for _ in range(3):
            b = device_run(emb, label, mem, memT, ml, count, kind, p, T, splits=S)
            assert all(torch.equal(a[k], b[k]) for k in ("out", "stats", "ell", "dxn")), S
        ref = oracle(a["xn"], label, mem, ml, count, kind, p)
        check(a, ref, kind, p, T, B, D, count, S or auto, f"splits={S} {kind} {str(T)[6:]}")
        res[S] = a
    assert all(torch.equal(res[0][k], res[auto][k]) for k in ("out", "stats", "ell", "dxn"))
    # the grid order (which workgroup gets which (anchor block, split)) changes no bit
    from pets_face_recognition_amd._hip import lib
    try:
        lib.pfr_set_tuning(b"pair_mem_order", 0)
        for S in (1, 3, 7):
            b = device_run(emb, label, mem, memT, ml, count, kind, p, T, splits=S)
            assert all(torch.equal(res[S][k], b[k]) for k in ("out", "stats", "ell", "dxn")), S
    finally:
        lib.pfr_set_tuning(b"pair_mem_order", 1)


@pytest.mark.parametrize("T", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_empty_ring_matches_the_batch_kernels(kind, T):
    """count = 0 through the new kernels against pfr_pair_loss_fwd / _bwd: both within the bounds of the same oracle, the same flags and A;
    PairLoss(memory=0) on the device is the batch path, bit for bit"""
    B, D, M = 70, 40, 96
    p = KINDS[kind]
    g = torch.Generator().manual_seed(31)
    emb = torch.randn(B, D, generator=g)
    label = layouts(B, 5)["mixed"]
    mem, memT = make_ring(M, 0, D, T, 32)
    ml = mem_labels(label, M, "shared", 33)
    o = ops()
    r = device_run(emb, label, mem, memT, ml, 0, kind, p, T)
    out, stats, ell = o.pair_loss_fwd(r["xn"], r["y"], kind, **p)
    dxn = o.pair_loss_bwd(r["xn"], r["xnT"], r["y"], stats, out, kind, grad_scale_dev=torch.tensor(UP, device=DEV), **p)
    old = dict(r, out=out.cpu(), stats=stats.cpu(), ell=ell.cpu(), dxn=dxn.cpu())
    ref = oracle(r["xn"], label, mem, ml, 0, kind, p)
    check(r, ref, kind, p, T, B, D, 0, 1, f"count=0 new {kind}")
    check(old, ref, kind, p, T, B, D, 0, 1, f"count=0 old {kind}")
    assert torch.equal(r["stats"][:, 3], old["stats"][:, 3]) and r["out"][2] == old["out"][2]
    e1, e2 = emb.to(DEV).requires_grad_(True), emb.to(DEV).requires_grad_(True)
    l1 = PairLoss(kind, memory=0, compute_dtype=T, **p)(e1, r["y"])
    l1.backward()
    xn, xnT, inv = o.l2norm_fwd(e2.detach(), T, want_t=True, ldt=(B + 31) // 32 * 32)
    out2, stats2, _ = o.pair_loss_fwd(xn, r["y"], kind, **p)
    d2 = o.l2norm_bwd(e2.detach(), inv, o.pair_loss_bwd(xn, xnT, r["y"], stats2, out2, kind, grad_scale_dev=torch.ones((), device=DEV), **p), torch.float32)
    assert torch.equal(l1.detach(), out2[0]) and torch.equal(e1.grad, d2)


@pytest.mark.parametrize("T", DTYPES, ids=["fp32", "bf16"])
def test_push_follows_the_cpu_ring(T):
    """the sequence of the host ring test (B = 37, M = 96, five pushes, the third wraps inside a batch): the device ring equals the CPU ring
    bit for bit after every push"""
    B, M, D = 37, 96, 40
    dev, cpu = PairLoss("supcon", memory=M), PairLoss("supcon", memory=M)
    g = torch.Generator().manual_seed(5)
    for step in range(5):
        xn = ops().l2norm_fwd(torch.randn(B, D, generator=g).to(DEV), T)[0]
        y = torch.randint(-5, 50, (B,), generator=g)
        dev.push(xn, y.to(DEV))
        cpu.push(xn.cpu(), y)
        torch.cuda.synchronize()
        assert (dev.head, dev.count, dev.generation) == (cpu.head, cpu.count, cpu.generation) == ((step + 1) * B % M, min((step + 1) * B, M), step + 1)
        assert dev.mem.dtype == T and torch.equal(dev.mem.cpu(), cpu.mem) and torch.equal(dev.memT.cpu(), cpu.memT)
        assert torch.equal(dev.mem_label.cpu(), cpu.mem_label)
        assert torch.equal(dev.memT[:, :dev.count], dev.mem[:dev.count].t()) and (dev.memT[:, dev.count:] == 0).all()


@pytest.mark.parametrize("T", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_edge_inputs(kind, T):
    """gamma = 256 / tau = 0.02; a slot identical to a batch row (s = 1) as a positive and as a negative; a zero row in the memory; a host
    and a device upstream factor together"""
    B, D, M, count = 70, 40, 128, 100
    g = torch.Generator().manual_seed(7)
    emb = torch.randn(B, D, generator=g)
    emb[5] = 0.0
    label = torch.randint(0, 9, (B,), generator=g)
    p = dict(m=0.25, gamma=256.0) if kind == "circle" else dict(tau=0.02)
    xn = ops().l2norm_fwd(emb.to(DEV), T)[0]
    mem, memT = make_ring(M, count, D, T, 8)
    ml = mem_labels(label, M, "shared", 9)
    mem[0], mem[1], mem[2] = xn[0], xn[0], 0.0
    ml[0], ml[1] = label[0], label[0] + 100
    memT[:, :count] = mem[:count].t()
    r = device_run(emb, label, mem, memT, ml, count, kind, p, T, up=-1.5, grad_scale=2.0)
    S = ops().pair_mem_splits(B, count, D)
    ref = oracle(r["xn"], label, mem, ml, count, kind, p, up=-3.0)
    check(r, ref, kind, p, T, B, D, count, S, f"edge {kind} {str(T)[6:]}")


@pytest.mark.parametrize("kind", list(KINDS))
def test_module_chain_and_guard(kind):
    """three training calls with M = 64, B = 20: the module's loss and embedding gradient are the kernel-level results of the same calls on a
    ring pushed by hand, bit for bit; the chain matches the CPU module in float64; the generation guard raises on the device path too"""
    B, D, M, T = 20, 64, 64, torch.bfloat16
    p = KINDS[kind]
    o = ops()
    g = torch.Generator().manual_seed(9)
    mod = PairLoss(kind, memory=M, compute_dtype=T, **p).to(DEV).train()
    ref_mod = PairLoss(kind, memory=M, **p).train()
    hand = PairLoss(kind, memory=M, **p)                    # a ring of its own, pushed by hand
    prev = None
    for step in range(3):
        emb = torch.randn(B, D, generator=g)
        label = torch.randint(0, 6, (B,), generator=g)
        e = emb.to(DEV).requires_grad_(True)
        y = label.to(DEV)
        loss = mod(e, y)
        loss.backward()
        # by hand
        if prev is not None:
            hand.push(*prev)
        xn, xnT, inv = o.l2norm_fwd(e.detach(), T, want_t=True, ldt=(B + 31) // 32 * 32)
        hand._ensure(xn)
        out, stats, _ = o.pair_mem_loss_fwd(xn, y, hand.mem, hand.mem_label, hand.count, kind, **p)
        dxn = o.pair_mem_loss_bwd(xn, xnT, y, hand.mem, hand.memT, hand.mem_label, hand.count, stats, out, kind,
                                  grad_scale_dev=torch.ones((), device=DEV), **p)
        demb = o.l2norm_bwd(e.detach(), inv, dxn, torch.float32)
        prev = (xn, y)
        assert (mod.count, mod.head, mod.generation) == (hand.count, hand.head, hand.generation) == (step * B, step * B % M, step)
        assert loss.shape == () and torch.equal(loss.detach(), out[0]) and torch.equal(e.grad, demb)
        # float64 on the CPU, normalisation included (bf16 operands: 2^-8 on a score)
        e64 = emb.double().requires_grad_(True)
        ref = ref_mod(e64, label)
        ref.backward()
        assert abs(loss.item() - ref.item()) < 2 * slope_of(kind, p) * 2.0 ** -8
        assert torch.isfinite(e.grad).all()
        if e64.grad.abs().sum() > 0:
            assert torch.nn.functional.cosine_similarity(e.grad.cpu().double().flatten(), e64.grad.flatten(), dim=0) > 0.99
    assert torch.equal(mod.mem[:2 * B].cpu(), hand.mem[:2 * B].cpu()) and list(mod.state_dict()) == []
    # eval: no push; then two forwards before the first backward
    mod.eval()
    mod(emb.to(DEV), y)
    assert mod.generation == 2
    mod.train()
    l1 = mod(emb.to(DEV).requires_grad_(True), y)
    l2 = mod(emb.to(DEV).requires_grad_(True), y)
    with pytest.raises(RuntimeError, match="generation"):
        l1.backward()
    l2.backward()
    torch.cuda.synchronize()


def test_centre_free_training_steps_with_memory(tmp_path, monkeypatch, capsys):
    """two PairMetricLearning steps through the Controller and the Trainer with pair_loss=dict(kind='supcon', memory=64), pk = (4, 4): the
    loss line reports loss_pair and the ring holds one batch after the second step's forward"""
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
         limit_train_batches=2, n_pairs=10, compute_dtype=torch.float32, pair_loss=dict(kind='supcon', tau=0.1, memory=64), pk=(4, 4),
         centre_free=True)

    class Cfg(dict):
        __getattr__ = dict.get

    torch.manual_seed(11)
    ctrl = Controller(Cfg(ns))
    assert isinstance(ctrl.model_loss, PairMetricLearning) and ctrl.model_loss.pair_loss.memory == 64
    t = Trainer(gpus=[0], max_epochs=1, check_val_every_n_epoch=100, prefetch_batches=0, limit_train_batches=2, log_every_n_steps=1)
    t.fit(ctrl)
    torch.cuda.synchronize()
    ring = ctrl.model_loss.pair_loss
    assert t.global_step == 2 and len(t.loss_history) == 2 and t.pair_loss_history == t.loss_history
    assert (ring.count, ring.head, ring.generation) == (16, 16, 1) and ring.mem.is_cuda and ring.mem.shape[0] == 64
    assert torch.isfinite(ring.mem[:16]).all() and ((ring.mem[:16].float().norm(dim=1) - 1).abs() < 1e-2).all()
    assert all(0 < v < 50 for v in t.loss_history) and all(torch.isfinite(p).all() for p in ctrl.parameters())
    assert "loss_pair" in capsys.readouterr().out
