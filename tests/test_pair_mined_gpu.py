"""The mined pair losses on the device (csrc/pfr_pairmine.hip: batch-hard triplet, Multi-Similarity) against the float64 CPU form of the
contract (losses/pair.py: pair_mined_parts), by the scheme of tests/test_pair_loss_gpu.py and tests/test_pair_memory_gpu.py: the oracle
is evaluated in float64 ON THE OPERAND BITS, every element is compared (extremes, partner numbers, validity, kept counts, the statistics,
l_i, the scalar, A and every component of dê), the upstream gradient 0.75 is a device scalar, a NaN guard row stands behind dê and the
ring slots >= count are NaN.

Mining and the hinge are discontinuous, so the inputs are such that no decision can differ between the device and float64:
  exact cases     rows handed in as ê directly: unit rows of four entries +-1/2, or one +-1/2 and twelve +-1/4 (D >= 16).  Every product and
                  every partial sum of a score is a multiple of 2^-4 below 2: exact in fp32 (and the rows are exact in bf16), so the device
                  scores EQUAL the float64 scores; epsilon, m and the base are dyadic, so s + epsilon, s - epsilon, s_n* - s_p* + m are
                  exact too.  Extremes, numbers and kept counts must match exactly, under heavy ties (most scores are 0).
  Gaussian cases  normalised Gaussian rows; a device score is within delta = D * 2^-24 of the float64 one (tests/test_pair_loss_gpu.py).
                  The test asserts FIRST, on the oracle alone, that no pair lies within 4 delta of its mining threshold, no z_i of the
                  hinge within 4 delta of 0 and no other candidate within 4 delta of an extreme (exact duplicates excepted: equal operand
                  bits give equal device scores and the tie rule decides).  The seeds were chosen on the CPU so that this holds with a
                  reserve (16 delta); nothing is skipped at run time.

Bounds (derived here, never tuned; observed / bound is printed and the largest ratios are recorded in profiles/pair_mined.txt).
u = 2^-24; expf / logf / log1pf are within 2 ulp = 4 u relative; ds = 0 (exact cases) or delta; n = B + count partners, nt tiles, S splits.
  batch_hard   z = fl(fl(s_n* - s_p*) + m): two roundings of numbers below 2 + m on top of the two scores: ez = 2 ds + 2 u (2 + m).
               gamma = 0: l = max(0, z): el = ez; f is 0 or 1: ef = 0.
               gamma > 0, t = fl(gamma z), |t| <= T = gamma (2 + m): softplus is 1-Lipschitz, expf and log1pf act on values <= 1 (8 u),
               the sum rounds at u (T + 1), the division at u l:  el = ez + (3 T + 10) u / gamma.   f = sigma(t), d ln f / dt <= 1:
               relative  ef = gamma ez + u T + 6 u  (expf 4 u, one add, one division).
  multi_sim.   logit x = fl(c fl(s - base)), |c| <= C = max(alpha, beta), |x| <= X = C (1 + |base|):  ex = C (ds + 2 u (1 + |base|)).
               An online log-sum-exp: every exponent fl(x - max) carries 2 X u, expf 4 u; a tile step is one rescale ((5 + 2 X) u) and 16
               adds; a merge (lane halves, 3 waves, S splits, the element 0) is (6 + 2 X) u; a lane sees at most nt tiles:
                 rho = (nt + S + 6) (22 + 2 X) u  relative on the sum, i.e. absolute on its logarithm;
               logf: 4 u log(n + 1); max + log: u (X + log(n + 1)):   eL = ex + rho + 4 u log(n + 1) + u (X + log(n + 1)).
               l = L_p / alpha + L_n / beta:  el = eL / alpha + eL / beta + 3 u lmax,  lmax = (X + log(n + 1)) (1 / alpha + 1 / beta).
               weight w = expf(fl(x - L)): relative  ew = ex + eL + u (X + log(n + 1)) + 4 u.
  scalar       the mean of l_i: strided partial sums, a lane tree, the waves, one division: el + (ceil(B / 256) + 10) u lmax.
  gradient     |ê_jd| <= 1.  G_rj = (W_rj + W_jr) scale with scale = fl(fl(grad_scale up) fl(1 / A)): 5 u with the add and the product.
               multi_sim.: the second product sums n terms in fp32, S slabs:  E_r = (ew + (n + 13 + S) u) sum_j |G|_rj, in bf16 plus
               2^-8 sum_j |G|_rj (G rounded once to bf16).   batch_hard: fp32 throughout, k_r reverse terms added one after the other:
               E_r = (ef + (k_r + 8) u) sum_j |G|_rj.   |G|_rj = |W_rj| + |W_jr| from the oracle (W_jr only for batch partners), times the
               upstream gradient.  A row whose bound is 0 must be exactly 0."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from pets_face_recognition_amd.losses.pair import PairLoss, pair_mined_parts

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTH = os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic")
U = 2.0 ** -24
UP = 0.75
DTYPES = [torch.float32, torch.bfloat16]
PARAMS = {"batch_hard": dict(m=0.25, gamma=0.0), "batch_hard_soft": dict(m=0.25, gamma=8.0),
          "multi_similarity": dict(alpha=2.0, beta=50.0, base=0.5, epsilon=0.125)}
RATIOS = {}
# Gaussian cases: (B, D, with ring, dtype) -> the first seed, searched on the CPU, with a 16 delta reserve in every layout and for every kind
SEEDS = {(129, 40, False, "float32"): 2, (129, 40, False, "bfloat16"): 3, (129, 40, True, "float32"): 3, (129, 40, True, "bfloat16"): 3}    # others: 1


def ops():
    from pets_face_recognition_amd._hip import ops as o
    return o


def kind_of(name):
    return "batch_hard" if name.startswith("batch_hard") else name


def layouts(B, seed):
    """label vectors [B] as in tests/test_pair_loss_gpu.py: class sizes 1-5 shuffled; all distinct; all equal; one class over a whole tile"""
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
        tile[t0:t0 + 32] = 10 ** 12
        out["tile"] = tile
    return out


def exact_rows(n, D, g):
    """n unit rows whose pairwise dot products are exact in fp32 and that are exact in bf16 (the docstring)"""
    x = torch.zeros(n, D)
    for r in range(n):
        perm = torch.randperm(D, generator=g)
        sign = torch.randint(0, 2, (13,), generator=g).float() * 2 - 1
        if D >= 16 and r % 3 == 2:
            x[r, perm[0]] = 0.5 * sign[0]
            x[r, perm[1:13]] = 0.25 * sign[1:13]
        else:
            x[r, perm[:4]] = 0.5 * sign[:4]
    return x


def gauss_rows(n, D, g, T):
    return F.normalize(torch.randn(n, D, generator=g), dim=1).to(T)


def make_ring(rows, M, T):
    """mem [M, D] with NaN at the slots >= count, memT [D, M] zero there"""
    count, D = rows.shape
    mem = torch.full((M, D), float("nan"), dtype=T, device=DEV)
    memT = torch.zeros((D, M), dtype=T, device=DEV)
    if count:
        mem[:count] = rows.to(DEV, T)
        memT[:, :count] = rows.to(DEV, T).t()
    return mem, memT


def device_run(xn_rows, label, ring, name, T, splits=0, up=UP, grad_scale=1.0):
    """xn_rows [B, D] (CPU) are handed in as ê; ring = None or (mem, memT, mem_label, count)"""
    o = ops()
    B, D = xn_rows.shape
    xn, y = xn_rows.to(DEV, T).contiguous(), label.to(DEV)
    xnT = torch.zeros((D, (B + 31) // 32 * 32), dtype=T, device=DEV)
    xnT[:, :B] = xn.t()
    kw = {} if ring is None else dict(mem=ring[0], mem_label=ring[2], count=ring[3])
    kwb = {} if ring is None else dict(kw, memT=ring[1])
    out, stats, ell = o.pair_mined_fwd(xn, y, kind_of(name), splits=splits, **kw, **PARAMS[name])
    dxn = torch.full((B + 1, D), float("nan"), device=DEV)
    o.pair_mined_bwd(xn, xnT, y, stats, out, kind_of(name), grad_scale=grad_scale, grad_scale_dev=torch.tensor(up, device=DEV), dxn=dxn[:B],
                     splits=splits, **kwb, **PARAMS[name])
    torch.cuda.synchronize()
    assert torch.isnan(dxn[B]).all()
    return dict(xn=xn, out=out.cpu(), stats=stats.cpu(), ell=ell.cpu(), dxn=dxn[:B].cpu())


def oracle(xn, label, mem_rows, mem_label, name, up=UP):
    """float64 on the operand bits: xn [B, D], mem_rows [count, D] (tensors of the compute dtype, any device)"""
    x = xn.cpu().double().requires_grad_(True)
    m = mem_rows.cpu().double()
    B, n = x.shape[0], x.shape[0] + m.shape[0]
    s = torch.cat([x @ x.t(), x @ m.t()], 1)
    s.retain_grad()
    same = label[:, None] == torch.cat([label, mem_label.cpu()])[None, :]
    eye = torch.cat([torch.eye(B, dtype=torch.bool), torch.zeros(B, n - B, dtype=torch.bool)], 1)
    pos, neg = same & ~eye, ~same
    r = pair_mined_parts(s, pos, neg, kind_of(name), **PARAMS[name])
    A = int(r["valid"].sum())
    loss = r["rows"].sum() / max(A, 1)
    loss.backward()
    W = (s.grad if s.grad is not None else torch.zeros_like(s)) * up
    absG = W.abs()
    absG[:, :B] += W[:, :B].abs().t()
    dx = (x.grad if x.grad is not None else torch.zeros_like(x)) * up
    return dict(r, s=s.detach(), pos=pos, neg=neg, A=A, loss=loss.item(), dxn=dx, W=W, absG=absG, rows=r["rows"].detach())


def decision_margin(ref, name):
    """the smallest distance, over the valid anchors, of a score to a decision boundary (exact duplicates of an extreme excepted)"""
    p, s = PARAMS[name], ref["s"]
    inf = torch.tensor(float("inf"), dtype=torch.float64)
    v = ref["valid"][:, None]
    gp = torch.where(ref["pos"] & v, s - ref["sp"][:, None], inf)
    gn = torch.where(ref["neg"] & v, ref["sn"][:, None] - s, inf)
    gaps = [torch.where(gp == 0, inf, gp).min(), torch.where(gn == 0, inf, gn).min()]
    if name == "batch_hard":
        gaps.append(torch.where(ref["valid"], ref["a"].abs(), inf).min())
    if name == "multi_similarity":
        gaps.append(torch.where(ref["neg"] & v, (s + p["epsilon"] - ref["sp"][:, None]).abs(), inf).min())
        gaps.append(torch.where(ref["pos"] & v, (s - p["epsilon"] - ref["sn"][:, None]).abs(), inf).min())
    return min(float(g) for g in gaps)


def bounds(name, B, count, D, S, exact):
    """-> dict of the docstring's bounds"""
    p = PARAMS[name]
    n, nt = B + count, (B + 31) // 32 + (count + 31) // 32
    ds = 0.0 if exact else D * U
    if kind_of(name) == "batch_hard":
        m, g = p["m"], p["gamma"]
        ez = 2 * ds + 2 * U * (2 + m)
        Tm = g * (2 + m)
        el = ez if g == 0 else ez + (3 * Tm + 10) * U / g
        ef = 0.0 if g == 0 else g * ez + U * Tm + 6 * U
        lmax = 2 + m + (1.0 / g if g else 0.0)
        return dict(ds=ds, ea=ez, eb=ef, el=el, eloss=el + (math.ceil(B / 256) + 10) * U * lmax, cg=ef + 8 * U)
    C = max(p["alpha"], p["beta"])
    X = C * (1 + abs(p["base"]))
    ex = C * (ds + 2 * U * (1 + abs(p["base"])))
    rho = (nt + S + 6) * (22 + 2 * X) * U
    ln = math.log(n + 1)
    eL = ex + rho + 4 * U * ln + U * (X + ln)
    lmax = (X + ln) * (1 / p["alpha"] + 1 / p["beta"])
    el = eL / p["alpha"] + eL / p["beta"] + 3 * U * lmax
    ew = ex + eL + U * (X + ln) + 4 * U
    return dict(ds=ds, ea=eL, eb=eL, el=el, eloss=el + (math.ceil(B / 256) + 10) * U * lmax, cg=ew + (n + 13 + S) * U)


def check(r, ref, name, T, B, count, D, S, exact, tag):
    bd = bounds(name, B, count, D, S, exact)
    st, sti = r["stats"], r["stats"].view(torch.int32)
    valid = ref["valid"]
    # decisions: exactly
    assert st[:, 7].bool().tolist() == valid.tolist() and set(st[:, 7].tolist()) <= {0.0, 1.0}, tag
    assert sti[:, 2].tolist() == ref["ip"].tolist() and sti[:, 3].tolist() == ref["inn"].tolist(), tag
    assert r["out"][2].item() == float(ref["A"]), tag
    assert abs(r["out"][1].item() - (1.0 / ref["A"] if ref["A"] else 0.0)) <= 2 * U / max(ref["A"], 1), tag
    kept = ref["keep"].sum(1) if name == "multi_similarity" else torch.zeros(B, dtype=torch.int64)
    assert st[:, 6].tolist() == kept.double().tolist(), tag
    assert (st[~valid][:, [0, 1, 4, 5, 6, 7]] == 0).all() and (sti[~valid][:, 2:4] == -1).all() and (r["ell"][~valid] == 0).all(), tag
    fl = st[:, [0, 1, 4, 5, 6, 7]]
    assert torch.isfinite(r["out"]).all() and torch.isfinite(r["ell"]).all() and torch.isfinite(r["dxn"]).all() and torch.isfinite(fl).all(), tag
    # extremes: equal in the exact cases, within delta otherwise
    e_s = max((st[:, 0].double() - ref["sp"]).abs().max().item(), (st[:, 1].double() - ref["sn"]).abs().max().item())
    assert e_s <= bd["ds"], (tag, e_s)
    # statistics, rows, scalar
    e_a = (st[:, 4].double() - ref["a"]).abs().max().item()
    if kind_of(name) == "batch_hard":                   # f: relative
        e_b = ((st[:, 5].double() - ref["b"]).abs() / ref["b"].clamp_min(1e-300)).max().item()
    else:
        e_b = (st[:, 5].double() - ref["b"]).abs().max().item()
    e_rows = (r["ell"].double() - ref["rows"]).abs().max().item()
    e_loss = abs(r["out"][0].item() - ref["loss"])
    # gradient, per row
    G1 = ref["absG"].sum(1)
    k_r = (ref["W"][:, :B] != 0).sum(0).double()
    coef = bd["cg"] + (k_r * U if kind_of(name) == "batch_hard" else 0.0)
    E = coef * G1
    if T == torch.bfloat16 and name == "multi_similarity":
        E = E + 2.0 ** -8 * G1
    err = (r["dxn"].double() - ref["dxn"]).abs().max(1).values
    live = E > 0
    ratio_g = (err[live] / E[live]).max().item() if live.any() else 0.0
    key = str(T).split(".")[1]
    for what, v, b in (("a", e_a, bd["ea"]), ("b", e_b, bd["eb"]), ("rows", e_rows, bd["el"]), ("loss", e_loss, bd["eloss"]), ("grad", ratio_g, 1.0)):
        if b > 0:
            RATIOS[(name, what, key)] = max(RATIOS.get((name, what, key), 0.0), v / b)
    print(f"{tag}: stats {e_a:.2e}/{bd['ea']:.2e} {e_b:.2e}/{bd['eb']:.2e}  l_i {e_rows:.2e}/{bd['el']:.2e}  loss {e_loss:.2e}/{bd['eloss']:.2e}"
          f"  grad err/bound {ratio_g:.3f}")
    assert e_a <= bd["ea"] and e_b <= bd["eb"], tag
    assert e_rows <= bd["el"] and e_loss <= bd["eloss"], tag
    assert (err <= E).all(), (tag, ratio_g)            # (a row whose bound is 0 must be exactly 0)
    if ref["A"] == 0:
        assert r["out"][0].item() == 0.0 and (r["dxn"] == 0).all(), tag


def tiles(B, count):
    return (B + 31) // 32 + (count + 31) // 32


def resolve(splits, B, count, D):
    return splits or ops().pair_mined_splits(B, count, D)


# ------------------------------------------------------------------------------------------------ 1. exact operands
@pytest.mark.parametrize("D", [8, 40, 512])
@pytest.mark.parametrize("name", list(PARAMS))
def test_exact_operands(name, D):
    """B in {1, 2, 37, 129, 200} x fp32 / bf16 x (no ring, M = 64 with count 0 / 33 / 64) x splits (auto, 1, 3, one beyond the tile count):
    one oracle per (B, ring), the same for both dtypes (the rows are exact in bf16) and every splits"""
    for B in (1, 2, 37, 129, 200):
        g = torch.Generator().manual_seed(100 * B + D)
        rows = exact_rows(B, D, g)
        if B >= 37:
            rows[B - 1] = rows[3]                        # a duplicated row: equal scores, the smaller number must win
        label = layouts(B, B + D)["mixed"]
        ring_rows = exact_rows(64, D, g)
        ring_rows[5] = rows[0]                           # a slot identical to a batch row
        ml = label[torch.randint(0, B, (64,), generator=g)]
        for M, count in ((0, 0), (64, 0), (64, 33), (64, 64)):
            ref = oracle(rows, label, ring_rows[:count], ml[:count], name)
            for T in DTYPES:
                ring = None
                if M:
                    mem, memT = make_ring(ring_rows[:count], M, T)
                    ring = (mem, memT, ml.to(DEV), count)
                for splits in (0, 1, 3, tiles(B, count) + 1):
                    r = device_run(rows, label, ring, name, T, splits=splits)
                    S = resolve(splits, B, count, D)
                    check(r, ref, name, T, B, count, D, S, True, f"exact {name} {str(T)[6:]} B={B} D={D} M={M} count={count} S={S}")
    print("largest error / bound so far:", {k: round(v, 4) for k, v in RATIOS.items()})


# ------------------------------------------------------------------------------------------------ 2. Gaussian rows
def gauss_case(B, D, with_ring, T, seed):
    g = torch.Generator().manual_seed(seed)
    rows = gauss_rows(B, D, g, T)
    ring_rows = gauss_rows(33 if with_ring else 0, D, g, T)
    return rows, ring_rows, g


GAUSS = [(37, 8), (129, 8), (37, 40), (129, 40)]


def gauss_seed(B, D, with_ring, T):
    return SEEDS.get((B, D, with_ring, str(T).split(".")[1]), 1)


@pytest.mark.parametrize("T", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("with_ring", [False, True], ids=["batch", "ring"])
@pytest.mark.parametrize("B,D", GAUSS)
@pytest.mark.parametrize("name", list(PARAMS))
def test_gaussian_rows(name, B, D, with_ring, T):
    rows, ring_rows, g = gauss_case(B, D, with_ring, T, gauss_seed(B, D, with_ring, T))
    count = ring_rows.shape[0]
    delta = D * U
    for lname, label in layouts(B, B + D).items():
        ml = label[torch.randint(0, B, (64,), generator=torch.Generator().manual_seed(count + B))]
        ref = oracle(rows, label, ring_rows, ml[:count], name)
        margin = decision_margin(ref, name)
        assert margin > 4 * delta, (lname, margin, delta)           # on the oracle alone, before anything is compared
        ring = None
        if with_ring:
            mem, memT = make_ring(ring_rows, 64, T)
            ring = (mem, memT, ml.to(DEV), count)
        for splits in (0, 3):
            r = device_run(rows, label, ring, name, T, splits=splits)
            S = resolve(splits, B, count, D)
            check(r, ref, name, T, B, count, D, S, False, f"gauss {name} {str(T)[6:]} B={B} D={D} count={count} S={S} {lname}")
    print("largest error / bound so far:", {k: round(v, 4) for k, v in RATIOS.items()})


# ------------------------------------------------------------------------------------------------ 3. further cases
@pytest.mark.parametrize("T", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(PARAMS))
def test_same_bits_every_call_and_nan_beyond_count(name, T):
    """four calls give identical bits for every splits; extremes, numbers, validity, kept counts (and all of batch_hard) do not depend on
    splits; what the slots >= count hold (NaN, or finite rows with matching labels) changes no bit"""
    B, D, M, count = 70, 40, 64, 33
    g = torch.Generator().manual_seed(5)
    rows, ring_rows = exact_rows(B, D, g), exact_rows(M, D, g)
    label = layouts(B, 9)["mixed"]
    ml = label[torch.randint(0, B, (M,), generator=g)].to(DEV)
    mem, memT = make_ring(ring_rows[:count], M, T)
    res = {}
    for S in (0, 1, 2, 5):
        a = device_run(rows, label, (mem, memT, ml, count), name, T, splits=S)
        for _ in range(3):
            b = device_run(rows, label, (mem, memT, ml, count), name, T, splits=S)
            assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in ("out", "stats", "ell", "dxn")), S
        res[S] = a
    for S in (0, 2, 5):
        cols = [0, 1, 2, 3, 6, 7] if name == "multi_similarity" else list(range(8))
        assert torch.equal(res[S]["stats"].view(torch.int32)[:, cols], res[1]["stats"].view(torch.int32)[:, cols]), S
        if kind_of(name) == "batch_hard":
            assert all(torch.equal(res[S][k], res[1][k]) for k in ("out", "ell", "dxn")), S
    mem2 = mem.clone()
    mem2[count:] = ring_rows[count:].to(DEV, T)          # live-looking rows beyond count: never read as partners
    c = device_run(rows, label, (mem2, memT, ml, count), name, T, splits=2)
    assert all(torch.equal(c[k].view(torch.int32), res[2][k].view(torch.int32)) for k in ("out", "stats", "ell", "dxn"))
    from pets_face_recognition_amd._hip import lib
    try:                                                 # the grid order changes no bit
        lib.pfr_set_tuning(b"pair_mem_order", 0)
        d = device_run(rows, label, (mem, memT, ml, count), name, T, splits=5)
        assert all(torch.equal(d[k].view(torch.int32), res[5][k].view(torch.int32)) for k in ("out", "stats", "ell", "dxn"))
    finally:
        lib.pfr_set_tuning(b"pair_mem_order", 1)


@pytest.mark.parametrize("T", DTYPES, ids=["fp32", "bf16"])
def test_duplicated_row_the_smaller_number_wins(T):
    """rows 1, 2 and slot 0 are the same positive of anchor 0, rows 3, 4 and slot 1 the same negative: p* = 1, n* = 3; without the batch
    copies the slots win"""
    D = 16
    e = torch.zeros(6, D)
    e[0, 0] = 1.0
    e[1, 0], e[1, 1] = 0.5, 0.5
    e[2] = e[1]
    e[3, 0], e[3, 2] = 0.25, -0.5
    e[4] = e[3]
    e[5, 3] = 1.0
    label = torch.tensor([0, 0, 0, 1, 1, 2])
    ring_rows = torch.stack([e[1], e[3]] + [e[5]] * 31)
    ml = torch.tensor([0, 1] + [7] * 62)
    mem, memT = make_ring(ring_rows, 64, T)
    for name in ("batch_hard", "multi_similarity"):
        r = device_run(e, label, (mem, memT, ml.to(DEV), 33), name, T)
        ref = oracle(e, label, ring_rows, ml[:33], name)
        check(r, ref, name, T, 6, 33, D, 1, True, f"duplicates {name}")
        assert r["stats"].view(torch.int32)[0, 2:4].tolist() == [1, 3]
        lab2 = torch.tensor([0, 5, 6, 8, 9, 2])           # the batch copies are other identities now: only the slots are left
        r2 = device_run(e, lab2, (mem, memT, ml.to(DEV), 33), name, T)
        check(r2, oracle(e, lab2, ring_rows, ml[:33], name), name, T, 6, 33, D, 1, True, f"duplicates, slots {name}")
        assert r2["stats"].view(torch.int32)[0, 2:4].tolist() == [6, 1]      # slot 0 = number B + 0; rows 1 and 2 are the hardest negatives now


@pytest.mark.parametrize("T", DTYPES, ids=["fp32", "bf16"])
def test_large_beta_and_host_times_device_upstream(T):
    """beta = 256 stays finite and within the bounds; a host and a device upstream factor together"""
    B, D, count = 70, 40, 33
    g = torch.Generator().manual_seed(7)
    rows, ring_rows = exact_rows(B, D, g), exact_rows(count, D, g)
    label = layouts(B, 4)["mixed"]
    ml = label[torch.randint(0, B, (64,), generator=g)]
    mem, memT = make_ring(ring_rows, 64, T)
    old = PARAMS["multi_similarity"]
    PARAMS["multi_similarity"] = dict(alpha=64.0, beta=256.0, base=0.5, epsilon=0.125)
    try:
        for name in ("multi_similarity", "batch_hard_soft"):
            r = device_run(rows, label, (mem, memT, ml.to(DEV), count), name, T, up=-1.5, grad_scale=2.0)
            ref = oracle(rows, label, ring_rows, ml[:count], name, up=-3.0)
            check(r, ref, name, T, B, count, D, resolve(0, B, count, D), True, f"edge {name} {str(T)[6:]}")
    finally:
        PARAMS["multi_similarity"] = old


@pytest.mark.parametrize("kind", ["batch_hard", "multi_similarity"])
def test_module_chain_and_guard(kind):
    """PairLoss(kind, memory=64) through pfr_l2norm_fwd, three training calls with B = 20: the deferred push, and loss and embedding
    gradient equal the kernel-level results of the same calls on a ring pushed by hand, bit for bit; memory = 0 is the batch-alone call;
    the generation guard raises"""
    B, D, M, T = 20, 64, 64, torch.bfloat16
    o = ops()
    g = torch.Generator().manual_seed(9)
    mod = PairLoss(kind, memory=M, compute_dtype=T).to(DEV).train()
    hand = PairLoss(kind, memory=M)
    p = mod.params
    prev = None
    for step in range(3):
        emb = torch.randn(B, D, generator=g)
        label = torch.randint(0, 6, (B,), generator=g)
        e, y = emb.to(DEV).requires_grad_(True), label.to(DEV)
        loss = mod(e, y)
        loss.backward()
        if prev is not None:
            hand.push(*prev)
        xn, xnT, inv = o.l2norm_fwd(e.detach(), T, want_t=True, ldt=(B + 31) // 32 * 32)
        hand._ensure(xn)
        out, stats, _ = o.pair_mined_fwd(xn, y, kind, mem=hand.mem, mem_label=hand.mem_label, count=hand.count, **p)
        dxn = o.pair_mined_bwd(xn, xnT, y, stats, out, kind, mem=hand.mem, memT=hand.memT, mem_label=hand.mem_label, count=hand.count,
                               grad_scale_dev=torch.ones((), device=DEV), **p)
        demb = o.l2norm_bwd(e.detach(), inv, dxn, torch.float32)
        prev = (xn, y)
        assert (mod.count, mod.head, mod.generation) == (hand.count, hand.head, hand.generation) == (step * B, step * B % M, step)
        assert loss.shape == () and torch.equal(loss.detach(), out[0]) and torch.equal(e.grad, demb)
        assert loss.item() > 0 and torch.isfinite(e.grad).all() and e.grad.abs().sum() > 0
    assert torch.equal(mod.mem[:2 * B].cpu(), hand.mem[:2 * B].cpu()) and list(mod.state_dict()) == []
    # memory = 0: the batch alone
    e0 = emb.to(DEV).requires_grad_(True)
    l0 = PairLoss(kind, compute_dtype=T)(e0, y)
    l0.backward()
    out0, stats0, _ = o.pair_mined_fwd(xn, y, kind, **p)
    d0 = o.l2norm_bwd(e.detach(), inv, o.pair_mined_bwd(xn, xnT, y, stats0, out0, kind, grad_scale_dev=torch.ones((), device=DEV), **p), torch.float32)
    assert torch.equal(l0.detach(), out0[0]) and torch.equal(e0.grad, d0)
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


@pytest.mark.parametrize("kind", ["batch_hard", "multi_similarity"])
def test_centre_free_training_step(kind, tmp_path, monkeypatch, capsys):
    """PairMetricLearning steps through the Controller and the Trainer with pk = (4, 4) and a memory of 64: the loss line reports loss_pair"""
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
         limit_train_batches=2, n_pairs=10, compute_dtype=torch.float32, pair_loss=dict(kind=kind, memory=64), pk=(4, 4), centre_free=True)

    class Cfg(dict):
        __getattr__ = dict.get

    torch.manual_seed(11)
    ctrl = Controller(Cfg(ns))
    assert isinstance(ctrl.model_loss, PairMetricLearning) and ctrl.model_loss.pair_loss.kind == kind
    t = Trainer(gpus=[0], max_epochs=1, check_val_every_n_epoch=100, prefetch_batches=0, limit_train_batches=2, log_every_n_steps=1)
    t.fit(ctrl)
    torch.cuda.synchronize()
    ring = ctrl.model_loss.pair_loss
    assert t.global_step == 2 and len(t.loss_history) == 2 and t.pair_loss_history == t.loss_history
    assert (ring.count, ring.head, ring.generation) == (16, 16, 1)
    assert all(0 < v < 50 for v in t.loss_history) and all(torch.isfinite(p).all() for p in ctrl.parameters())
    assert "loss_pair" in capsys.readouterr().out
