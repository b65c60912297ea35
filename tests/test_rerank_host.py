"""Host side of the k-reciprocal re-ranking (no GPU): pfr_rerank_row_capacity, the argument checks of the pfr_rerank_* entry points, the CPU
path of match.rerank against the dense fp64 oracle (tests/rerank_oracle.py), recall_at_k(rerank=None) and the opt-in keys of the Controller
and of eval_fe.py."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

from rerank_oracle import U, capacity, dist_bound, lists_from_rows, make_set, oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C-ABI
@pytest.mark.parametrize("k1", [1, 2, 5, 8, 20])
@pytest.mark.parametrize("k2", [1, 6])
def test_row_capacity_is_the_formula(k1, k2):
    from pets_face_recognition_amd.match import rerank_row_capacity
    kh = {1: 0, 2: 1, 5: 2, 8: 4, 20: 10}[k1]                  # round half to even: 0.5 -> 0, 2.5 -> 2
    E = (k1 + 1) + (k1 + 1) * (kh + 1)
    assert rerank_row_capacity(k1, k2) == (E, k2 * E) == capacity(k1, k2)
    assert rerank_row_capacity(3, 1)[0] == 4 + 4 * 3 and rerank_row_capacity(7, 1)[0] == 8 + 8 * 5    # 1.5 -> 2, 3.5 -> 4


def test_entry_points_declared_and_exported():
    import ctypes
    from pets_face_recognition_amd._hip.lib import LIB_PATH, parse_header
    protos = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    for name in ("pfr_rerank_row_capacity", "pfr_rerank_expand", "pfr_rerank_average", "pfr_rerank_score"):
        assert name in protos and hasattr(dll, name), name
    inc = open(os.path.join(os.path.dirname(LIB_PATH), "pfr_thunks_gen.inc")).read()
    assert '{"pfr_rerank_score", th_pfr_rerank_score}' in inc
    hdr = open(os.path.join(ROOT, "include", "pfr_hip.h")).read()
    assert "per-column maximum" in hdr and "RESTRICTED CANDIDATE LISTS" in hdr      # the two stated deviations are part of the header


def test_argument_errors_are_reported_not_crashed():
    """every call fails a geometry or null check before any pointer is looked at (16 is no address of anything)"""
    from pets_face_recognition_amd._hip import lib, PfrError
    P = 16
    with pytest.raises(PfrError, match="null pointer"):
        lib.pfr_rerank_row_capacity(20, 6, 0, 0)
    for k1, k2 in ((0, 1), (512, 1), (-3, 1), (20, 0)):
        with pytest.raises(PfrError):
            lib.pfr_rerank_row_capacity(k1, k2, P, P)
    E, E2 = capacity(20, 6)
    expand = lambda emb=P, N=8, D=64, nbr=P, k1=20, vi=P, vv=P, vc=P, cap=E: lib.pfr_rerank_expand(emb, N, D, nbr, k1, vi, vv, vc, cap, 0)
    for kw, msg in ((dict(k1=0), "k1"), (dict(k1=512), "k1"), (dict(cap=E - 1), "capacity"), (dict(emb=0), "null pointer"),
                    (dict(vc=0), "null pointer"), (dict(D=0), "shape"), (dict(N=-1), "shape"), (dict(k1=400, cap=1 << 20), "LDS")):
        with pytest.raises(PfrError, match=msg):
            expand(**kw)
    average = lambda nbr=P, N=8, k1=20, k2=6, vi=P, cap=E, qi=P, cap2=E2: lib.pfr_rerank_average(nbr, N, k1, k2, vi, P, P, cap, qi, P, P, cap2, 0)
    for kw, msg in ((dict(k1=0), "k1"), (dict(k2=0), "k2"), (dict(cap=E - 1), "capacity"), (dict(cap2=E2 - 1), "capacity"),
                    (dict(nbr=0), "null pointer"), (dict(qi=0), "null pointer"), (dict(k1=100, k2=64, cap=1 << 20, cap2=1 << 24), "LDS")):
        with pytest.raises(PfrError, match=msg):
            average(**kw)
    score = lambda qi=P, N=8, cap2=E2, rows=P, R=4, cand=P, kc=100, lam=0.3, k=10, dist=P: lib.pfr_rerank_score(qi, P, P, N, cap2, rows, R, cand,
                                                                                                                 P, kc, lam, k, dist, P, 0)
    for kw, msg in ((dict(kc=513), "kc"), (dict(kc=0), "kc"), (dict(k=101), "k="), (dict(k=0), "k="), (dict(lam=1.5), "lambda"),
                    (dict(lam=float("nan")), "lambda"), (dict(rows=0), "null pointer"), (dict(dist=0), "null pointer"), (dict(cap2=0), "shape"),
                    (dict(cap2=1 << 20), "LDS")):
        with pytest.raises(PfrError, match=msg):
            score(**kw)


# ---- the CPU path of match.rerank
@pytest.mark.parametrize("N", [1, 2, 7, 60])
@pytest.mark.parametrize("k1,k2,lam", [(5, 3, 0.3), (8, 1, 0.0), (3, 2, 1.0)])
def test_cpu_path_against_the_dense_oracle(N, k1, k2, lam):
    from pets_face_recognition_amd.match import rerank, rerank_inputs, rerank_lists
    D, k = 32, 10
    emb = make_set("clustered", N, D, seed=N + k1, k1=k1) * 3.0         # (any scale: rerank normalises)
    emb32, nbr, rows, cand, cand_cos, off = rerank_inputs(emb, k, k1=k1, candidates=None)
    assert off == 0 and nbr.shape == (N, k1 + 1) and cand.shape == (N, min(100, N - 1)) and torch.equal(nbr[:, 0], torch.arange(N).int())
    dist, idx = rerank(emb, k, k1=k1, k2=k2, lambda_value=lam)
    assert dist.shape == idx.shape == (N, k) and dist.dtype == torch.float32 and idx.dtype == torch.int32
    d2, i2 = rerank_lists(emb32, nbr, rows, cand, cand_cos, k, k1, k2, lam)
    assert torch.equal(dist, d2) and torch.equal(idx, i2)
    if N == 1:
        assert bool(torch.isinf(dist).all()) and bool((idx == -1).all())
        return
    O = oracle(emb32, nbr, rows, cand, cand_cos, k1, k2, lam)
    bound = dist_bound(D, k1, k2, lam)
    fin = O["final"]
    for r in range(N):
        nv = int(np.isfinite(fin[r]).sum())
        kk = min(k, nv)
        got_i, got_d = idx[r].numpy(), dist[r].double().numpy()
        assert (got_i[kk:] == -1).all() and np.isinf(got_d[kk:]).all()
        assert len(set(got_i[:kk])) == kk and r not in got_i[:kk]
        assert (np.diff(got_d[:kk]) >= 0).all()
        pos = [list(cand[r].numpy()).index(j) for j in got_i[:kk]]
        assert np.abs(got_d[:kk] - fin[r, pos]).max() <= bound
        assert np.abs(got_d[:kk] - np.sort(fin[r])[:kk]).max() <= bound
    if lam == 1.0:                        # the cosine order itself
        kk = min(k, N - 1)
        assert torch.equal(idx[:, :kk], cand[:, :kk]) and torch.equal(dist[:, :kk], 2 - 2 * cand_cos[:, :kk])


def test_cpu_path_gallery_form_and_limits():
    from pets_face_recognition_amd._hip import PfrError
    from pets_face_recognition_amd import match
    q, g = make_set("random", 6, 16, 1), make_set("random", 30, 16, 2)
    dist, idx = match.rerank(q, 5, k1=4, k2=2, emb_b=g, candidates=12)
    assert dist.shape == (6, 5) and int(idx.min()) >= 0 and int(idx.max()) < 30          # gallery numbering
    emb32, nbr, rows, cand, cand_cos, off = match.rerank_inputs(q, 5, k1=4, candidates=12, emb_b=g)
    assert off == 6 and emb32.shape[0] == 36 and int(cand.min()) >= 6 and rows.tolist() == list(range(6))
    O = oracle(emb32, nbr, rows, cand, cand_cos, 4, 2, 0.3)
    for r in range(6):
        pos = [cand[r].tolist().index(j + 6) for j in idx[r].tolist()]
        assert np.abs(dist[r].double().numpy() - O["final"][r, pos]).max() <= dist_bound(16, 4, 2, 0.3)
    x = make_set("random", 8, 16, 3)
    for kw in (dict(k=513), dict(k=5, k1=512), dict(k=5, k1=0), dict(k=5, k2=0), dict(k=5, candidates=513), dict(k=5, lambda_value=1.5)):
        with pytest.raises(PfrError):
            match.rerank(x, **kw)
    with pytest.raises(PfrError, match="dense"):
        match.rerank(torch.zeros(match.RERANK_CPU_MAX_ITEMS + 1, 4), 5, neighbors=(torch.zeros(match.RERANK_CPU_MAX_ITEMS + 1, 100),
                                                                                   torch.zeros(match.RERANK_CPU_MAX_ITEMS + 1, 100).int()))


def test_recall_at_k_without_rerank_is_unchanged_and_with_it_follows_the_oracle():
    """rerank=None is the current function.  With it the counts must EQUAL those of the oracle's order: the set (noisy classes of 3; chosen on the oracle alone) has
    no near-tie on a K boundary — the smallest gap between the K-th and the (K + 1)-th oracle distance is several times the derived bound, asserted below — and its
    re-ranked counts differ from the cosine-order counts and from 100 % at every K."""
    from oracle import match_ref
    from pets_face_recognition_amd.match import recall_at_k, rerank_inputs
    N, D, k1, k2, lam, ks = 60, 32, 6, 2, 0.3, (1, 5, 10)
    g = torch.Generator().manual_seed(10)
    cls = torch.arange(N) // 3
    emb = torch.randn(N // 3, D, generator=g)[cls] + 2.0 * torch.randn(N, D, generator=g)
    base = recall_at_k(emb, cls, ks)
    assert recall_at_k(emb, cls, ks, rerank=None) == base == match_ref.recall_at_k_matrix(emb, cls, ks)
    got = recall_at_k(emb, cls, ks, rerank=dict(k1=k1, k2=k2, lambda_value=lam))
    emb32, nbr, rows, cand, cand_cos, _ = rerank_inputs(emb, max(ks), k1=k1)
    fin = oracle(emb32, nbr, rows, cand, cand_cos, k1, k2, lam)["final"]
    srt = np.sort(fin, axis=1)
    assert min((srt[:, K] - srt[:, K - 1]).min() for K in ks) > 2 * dist_bound(D, k1, k2, lam)      # no row can fall either way
    ranked = np.take_along_axis(cand.numpy(), np.argsort(fin, axis=1, kind="stable"), 1)
    same = cls.numpy()[ranked] == cls.numpy()[:, None]
    want = {K: [int(same[:, :K].any(1).sum()), N] for K in ks}
    assert got == want
    assert all(want[K][0] != base[K][0] and want[K][0] < N for K in ks)


def test_cpu_path_skips_padding_inside_the_lists():
    """entries outside [0, N) in the middle of nbr / cand rows, and an output row outside the set: skipped, as the contract says"""
    from pets_face_recognition_amd.match import rerank_lists
    N, D, k1, k2, lam, k = 40, 32, 6, 3, 0.3, 12
    emb32 = make_set("clustered", N, D, seed=8, k1=k1)
    nbr, rows, cand, cand_cos = lists_from_rows(emb32, k1, 15)
    nbr, cand, rows = nbr.clone(), cand.clone(), rows.clone()
    for i, bad in zip(range(0, N, 3), [-1, N, 2 ** 30, -2 ** 31] * 4):
        nbr[i, 1 + i % k1] = bad
        nbr[(i + 1) % N, 2] = bad
    cand[5, 3], cand[6, 0], cand[7, 14], rows[9] = N, -5, 2 ** 30, N + 3
    O = oracle(emb32, nbr, rows, cand, cand_cos, k1, k2, lam)
    dist, idx = rerank_lists(emb32, nbr, rows, cand, cand_cos, k, k1, k2, lam)
    assert bool((idx[9] == -1).all()) and bool(torch.isinf(dist[9]).all())
    for r in range(N):
        nv = int(np.isfinite(O["final"][r]).sum())
        kk = min(k, nv)
        assert (idx[r, kk:] == -1).all() and bool(torch.isinf(dist[r, kk:]).all())
        assert np.abs(dist[r, :kk].double().numpy() - np.sort(O["final"][r])[:kk]).max(initial=0) <= dist_bound(D, k1, k2, lam)
        pos = [cand[r].tolist().index(j) for j in idx[r, :kk].tolist()]
        assert np.abs(dist[r, :kk].double().numpy() - O["final"][r, pos]).max(initial=0) <= dist_bound(D, k1, k2, lam)


# ---- Controller and eval_fe.py
def _controller(extra):
    from pets_face_recognition_amd.engine.controller import Controller
    g = torch.Generator().manual_seed(3)
    N = 60
    classes = torch.arange(N) // 3
    emb = torch.randn(20, 32, generator=g)[classes] + 0.5 * torch.randn(N, 32, generator=g)
    pairs = [(i, i + 1) for i in range(0, N, 3)] + [(i, (i + 7) % N) for i in range(0, N, 2)]
    plabels = [int(classes[a] == classes[b]) for a, b in pairs]

    class PG:
        corrected_indices = pairs
        labels = plabels

    def sim(ps):
        t1 = torch.stack([p[0] for p in ps]); t2 = torch.stack([p[1] for p in ps])
        return (torch.nn.functional.cosine_similarity(t1, t2) + 1) / 2
    sim._is_default_cosine = True

    class Cfg(dict):
        def pair_generator(self, i):
            return "Val", PG

    cfg = Cfg(thrs=[0.6, 0.8], k=[1, 5], far_thr=[0.1, 0.05], frr_thr=[0.1], img_dir=tempfile.mkdtemp(), **extra)
    cfg.similarity_f = sim
    cfg.match_dtype = torch.float32
    c = Controller.__new__(Controller)
    torch.nn.Module.__init__(c)
    c.logger, c.current_epoch, c.last_metrics, c.config = None, 0, {}, cfg
    perm = torch.randperm(N, generator=g)
    batches = [{"emb": emb[perm][i:i + 20], "label": classes[perm][i:i + 20], "index": perm[i:i + 20]} for i in range(0, N, 20)]
    return c, batches, emb, classes


@pytest.mark.parametrize("method,ks", [("_evaluate", (1, 5)), ("test_epoch_end", (10, 100))])
def test_controller_rerank_is_opt_in(method, ks):
    from pets_face_recognition_amd.match import recall_at_k
    c0, batches, emb, classes = _controller({})
    base = getattr(c0, method)([batches])["Val"]
    assert not any(k.startswith("Rerank") for k in base)
    rr = dict(k1=6, k2=2, lambda_value=0.3)
    c1, batches, _, _ = _controller({"rerank": rr})
    m = getattr(c1, method)([batches])["Val"]
    assert list(m.keys()) == list(base.keys()) + [f"Rerank Recall@K={k}" for k in ks]
    for k, v in base.items():                     # the existing metrics do not move
        assert m[k] == v or (v != v and m[k] != m[k]), k
    want = recall_at_k(emb, classes, ks, compute_dtype=torch.float32, rerank=rr)
    for k in ks:
        assert m[f"Rerank Recall@K={k}"] == want[k][0] / want[k][1]
    # all-pairs keys stay in front of the new ones
    c2, batches, _, _ = _controller({"rerank": rr, "all_pairs_far": []})
    keys = list(getattr(c2, method)([batches])["Val"].keys())
    assert keys == list(base.keys()) + ["AllPairs ROC AUC", "AllPairs EER"] + [f"Rerank Recall@K={k}" for k in ks]


def test_eval_fe_flag_reaches_the_config(monkeypatch):
    sys.path.insert(0, ROOT)
    import eval_fe
    seen = {}

    class FakeController:
        def __init__(self, config):
            seen["rerank"] = config.get("rerank")

    class FakeTrainer:
        def test(self, controller):
            return "tested"

    monkeypatch.setattr(eval_fe, "Controller", FakeController)
    monkeypatch.setattr(eval_fe, "configure_trainer", lambda *a, **k: FakeTrainer())
    with tempfile.TemporaryDirectory() as td:
        cfg = os.path.join(td, "cfg.py")
        open(cfg, "w").write("n_epochs = 1\ndevice = 'cpu'\n")
        assert eval_fe.main(["-c", cfg, "--rerank", "20", "6", "0.3"]) == "tested"
        assert seen["rerank"] == dict(k1=20, k2=6, lambda_value=0.3)
        assert eval_fe.main(["-c", cfg]) == "tested"
        assert seen["rerank"] is None


def test_rerank_config_sets_the_key():
    src = open(os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic", "fe_r18_mi355x_rerank.py")).read()
    assert "rerank = dict(k1=" in src and "_make(globals()" in src
