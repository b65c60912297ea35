"""Host side of the all-pairs verification (no GPU): the CPU path of match.pair_histogram against a double loop, HistStats on hand-made
tables (the far_points rule, eer, the NaN slot), its auroc against PairStats within the exact worth of the within-bin ties, the opt-in keys of
Controller._evaluate / test_epoch_end, eval_fe.py's flag, and the C-ABI declaration of pfr_pair_hist."""
import ctypes
import math
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _brute(S, ca, cb, bins, lo, inv_w, sym):
    """the contract, pair by pair, on the fp32 scores S[i][j]: x = (s - lo) * inv_w in fp32, clamp(floor), NaN -> slot bins"""
    t = np.zeros((2, bins + 1), dtype=np.int64)
    for i in range(S.shape[0]):
        for j in range(S.shape[1]):
            if sym and not i < j:
                continue
            s = F32(S[i, j])
            x = F32(F32(s - F32(lo)) * F32(inv_w))
            slot = bins if np.isnan(s) else int(min(max(math.floor(x), 0), bins - 1))
            t[int(ca[i] == cb[j]), slot] += 1
    return torch.tensor(t)


@pytest.mark.parametrize("bins,rng", [(16, (-1.0, 1.0)), (5, (-0.1, 0.3)), (4096, (-1.0, 1.0))])
def test_cpu_path_equals_double_loop(bins, rng):
    """random rows: the scores are the fp32 matmul of the normalised rows (the CPU path's definition), everything after them — bin rule,
    saturation, kinds, i < j — is redone pair by pair"""
    from pets_face_recognition_amd.match import pair_histogram
    g = torch.Generator().manual_seed(0)
    N = 40
    x, y = torch.randn(N, 16, generator=g), torch.randn(23, 16, generator=g)
    ca, cb = torch.randint(0, 5, (N,), generator=g), torch.randint(0, 5, (23,), generator=g)
    hist, lo, inv_w = pair_histogram(x, ca, bins=bins, range=rng)
    assert hist.dtype == torch.int64 and hist.shape == (2, bins + 1)
    assert inv_w == float(F32(bins) / (F32(rng[1]) - F32(rng[0]))) and lo == float(F32(rng[0]))
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    yn = y / y.norm(dim=1, keepdim=True).clamp_min(1e-12)
    want = _brute((xn @ xn.t()).numpy(), ca.numpy(), ca.numpy(), bins, lo, inv_w, True)
    assert int(hist.sum()) == N * (N - 1) // 2 and torch.equal(hist, want)
    h2, _, _ = pair_histogram(x, ca, y, cb, bins=bins, range=rng)
    want2 = _brute((xn @ yn.t()).numpy(), ca.numpy(), cb.numpy(), bins, lo, inv_w, False)
    assert int(h2.sum()) == N * 23 and torch.equal(h2, want2)


def test_cpu_path_exact_on_integer_rows_and_nan():
    from pets_face_recognition_amd.match import pair_histogram
    g = torch.Generator().manual_seed(1)
    N, D, bins = 40, 8, 64
    x = torch.randint(-2, 3, (N, D), generator=g).float()
    x[7, 2] = float("nan")
    c = torch.randint(0, 4, (N,), generator=g)
    hist, lo, inv_w = pair_histogram(x, c, bins=bins, range=(-32.0, 32.0), normalize=False, compute_dtype=torch.float32)
    S = (x.double() @ x.double().t()).float().numpy()      # integer dots: exact, whatever the summation order
    want = _brute(S, c.numpy(), c.numpy(), bins, lo, inv_w, True)
    assert torch.equal(hist, want) and int(hist[:, bins].sum()) == N - 1
    # saturation: a narrow range puts everything outside it into the end bins
    h2, lo2, w2 = pair_histogram(x, c, bins=4, range=(-1.0, 1.0), normalize=False)
    assert torch.equal(h2, _brute(S, c.numpy(), c.numpy(), 4, lo2, w2, True))
    with pytest.raises(Exception):
        pair_histogram(x, c, bins=0)
    with pytest.raises(Exception):
        pair_histogram(x, c, bins=8193)
    with pytest.raises(Exception):
        pair_histogram(x, c, compute_dtype=torch.float16)


# ---- HistStats on hand-made tables
def _table():
    # bins = 4 over [0, 4): impostors pile low, genuines high; 3 NaN pairs that must count nowhere
    return torch.tensor([[500, 300, 150, 50, 2],
                         [0, 10, 30, 60, 1]]), 0.0, 1.0


def test_hist_stats_counts_and_far_rule():
    from pets_face_recognition_amd.engine.metrics import HistStats
    h, lo, inv_w = _table()
    hs = HistStats(h, lo, inv_w, to_similarity=False)
    assert (hs.n_neg, hs.n_pos, hs.n_nan) == (1000, 100, 3)
    assert hs.fp.tolist() == [1000, 500, 200, 50, 0] and hs.tp.tolist() == [100, 100, 90, 60, 0]
    st = hs.stats_at_bin(2)
    assert (st["tp"], st["fp"], st["fn"], st["tn"]) == (90, 200, 10, 800)
    assert st["threshold"] == 2.0 and st["tar"] == 0.9 and st["far"] == 0.2
    pts = hs.far_points([0.5, 0.3, 0.2, 0.05, 0.01, 0.0, 1.0])
    assert pts[0.5] == (1.0, 1.0, 0.5)            # exact equality FP / n_neg == far qualifies
    assert pts[0.3] == (0.9, 2.0, 0.2)            # most permissive threshold that does not exceed the far
    assert pts[0.2] == (0.9, 2.0, 0.2)
    assert pts[0.05] == (0.6, 3.0, 0.05)
    assert pts[0.01] == (0.0, 4.0, 0.0)           # no bin reaches it: the operating point that accepts nothing
    assert pts[0.0] == (0.0, 4.0, 0.0)
    assert pts[1.0] == (1.0, 0.0, 1.0)
    # the NaN slot changes no rate
    h2 = h.clone()
    h2[:, 4] = 0
    hs2 = HistStats(h2, lo, inv_w, to_similarity=False)
    assert hs2.n_nan == 0 and hs2.auroc() == hs.auroc() and hs2.eer() == hs.eer() and hs2.far_points([0.05]) == hs.far_points([0.05])
    # similarity thresholds: (cos + 1) / 2 of the bin's lower edge
    hs3 = HistStats(torch.zeros(2, 9, dtype=torch.long) + 1, -1.0, 4.0)
    assert hs3.threshold(0) == 0.0 and hs3.threshold(4) == 0.5 and hs3.threshold(8) == 1.0


def test_hist_stats_eer_and_auroc_by_hand():
    from pets_face_recognition_amd.engine.metrics import HistStats
    h, lo, inv_w = _table()
    hs = HistStats(h, lo, inv_w, to_similarity=False)
    # FAR(b) = 1, .5, .2, .05, 0;  FRR(b) = 0, 0, .1, .4, 1: the closest pair is b = 2 -> (0.2 + 0.1) / 2
    assert abs(hs.eer() - 0.15) < 1e-15
    # AUROC with within-bin ties worth one half: (sum_b pos_b * (neg below b) + pos_b * neg_b / 2) / (n_pos n_neg)
    neg, pos = h[0, :4].double(), h[1, :4].double()
    below = torch.cumsum(neg, 0) - neg
    want = float(((pos * below).sum() + 0.5 * (pos * neg).sum()) / (100 * 1000))
    assert abs(hs.auroc() - want) < 1e-15
    # perfectly separated and perfectly mixed tables
    assert HistStats(torch.tensor([[5, 0, 0], [0, 7, 0]]), 0.0, 1.0).auroc() == 1.0
    assert HistStats(torch.tensor([[5, 0, 0], [0, 7, 0]]), 0.0, 1.0).eer() == 0.0
    assert HistStats(torch.tensor([[4, 4, 0], [3, 3, 0]]), 0.0, 1.0).auroc() == 0.5


def test_hist_auroc_against_pair_stats_within_tie_mass():
    """the two AUROCs differ by the pairs that share a bin: at most (1/2) sum_b pos_b neg_b / (n_pos n_neg), computed from the table itself"""
    from pets_face_recognition_amd.engine.metrics import HistStats, PairStats
    from pets_face_recognition_amd.match import pair_histogram
    g = torch.Generator().manual_seed(2)
    N = 120
    cls = torch.randint(0, 12, (N,), generator=g)
    x = torch.randn(12, 32, generator=g)[cls] + 0.8 * torch.randn(N, 32, generator=g)
    xn = torch.nn.functional.normalize(x, dim=1, eps=1e-12)
    iu = torch.triu_indices(N, N, 1)
    scores = (xn @ xn.t())[iu[0], iu[1]]
    labels = (cls[iu[0]] == cls[iu[1]]).long()
    exact = PairStats(scores, labels).auroc()
    for bins in (16, 256, 4096):
        hist, lo, inv_w = pair_histogram(x, cls, bins=bins)
        hs = HistStats(hist, lo, inv_w)
        assert (hs.n_pos, hs.n_neg) == (int(labels.sum()), int((1 - labels).sum()))
        tol = 0.5 * float((hs.pos.double() * hs.neg.double()).sum()) / (hs.n_pos * hs.n_neg)
        assert abs(hs.auroc() - exact) <= tol + 1e-12, (bins, hs.auroc(), exact, tol)
    assert tol < 1e-3      # (4096 bins: the tie mass itself is small)


# ---- Controller
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

    td = tempfile.mkdtemp()
    cfg = Cfg(thrs=[0.6, 0.8], k=[1, 5], far_thr=[0.1, 0.05], frr_thr=[0.1], img_dir=td, **extra)
    cfg.similarity_f = sim
    cfg.match_dtype = torch.float32
    c = Controller.__new__(Controller)
    torch.nn.Module.__init__(c)
    c.logger, c.current_epoch, c.last_metrics, c.config = None, 0, {}, cfg
    perm = torch.randperm(N, generator=g)
    batches = [{"emb": emb[perm][i:i + 20], "label": classes[perm][i:i + 20], "index": perm[i:i + 20]} for i in range(0, N, 20)]
    return c, batches, emb, classes


def _all_pairs_keys(fars):
    return (["AllPairs ROC AUC", "AllPairs EER"] + [f"AllPairs TAR@FAR={f}" for f in fars] + [f"AllPairs TH@FAR={f}" for f in fars])


@pytest.mark.parametrize("method", ["_evaluate", "test_epoch_end"])
def test_controller_all_pairs_is_opt_in(method):
    from pets_face_recognition_amd.engine.metrics import HistStats
    from pets_face_recognition_amd.match import pair_histogram
    c0, batches, emb, classes = _controller({})
    base = getattr(c0, method)([batches])["Val"]
    assert not any(k.startswith("AllPairs") for k in base)
    fars = [0.1, 0.01, 1e-3]
    c1, batches, _, _ = _controller({"all_pairs_far": fars, "all_pairs_bins": 512})
    m = getattr(c1, method)([batches])["Val"]
    keys = list(m.keys())
    assert keys == list(base.keys()) + _all_pairs_keys(fars)
    for k, v in base.items():                     # the existing metrics do not move
        assert m[k] == v or (v != v and m[k] != m[k]), k
    hist, lo, inv_w = pair_histogram(emb, classes, bins=512, compute_dtype=torch.float32)
    hs = HistStats(hist, lo, inv_w)
    assert m["AllPairs ROC AUC"] == hs.auroc() and m["AllPairs EER"] == hs.eer()
    pts = hs.far_points(fars)
    for f in fars:
        assert m[f"AllPairs TAR@FAR={f}"] == pts[f][0] and m[f"AllPairs TH@FAR={f}"] == pts[f][1]
        assert 0.0 <= m[f"AllPairs TH@FAR={f}"] <= 1.0
    assert hs.n_pos + hs.n_neg == 60 * 59 // 2 and hs.n_pos == 60
    # an empty list still opts in: the two rate-free keys only
    c2, batches, _, _ = _controller({"all_pairs_far": []})
    assert list(getattr(c2, method)([batches])["Val"].keys()) == list(base.keys()) + _all_pairs_keys([])


def test_eval_fe_flag_reaches_the_config(monkeypatch):
    sys.path.insert(0, ROOT)
    import eval_fe
    seen = {}

    class FakeController:
        def __init__(self, config):
            seen["far"] = config.get("all_pairs_far")

    class FakeTrainer:
        def test(self, controller):
            return "tested"

    monkeypatch.setattr(eval_fe, "Controller", FakeController)
    monkeypatch.setattr(eval_fe, "configure_trainer", lambda *a, **k: FakeTrainer())
    with tempfile.TemporaryDirectory() as td:
        cfg = os.path.join(td, "cfg.py")
        open(cfg, "w").write("n_epochs = 1\ndevice = 'cpu'\n")
        assert eval_fe.main(["-c", cfg, "--all-pairs-far", "1e-4", "1e-6"]) == "tested"
        assert seen["far"] == [1e-4, 1e-6]
        assert eval_fe.main(["-c", cfg]) == "tested"
        assert seen["far"] is None


def test_all_pairs_config_sets_the_key():
    src = open(os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic", "fe_r18_mi355x_allpairs.py")).read()
    assert "all_pairs_far" in src and "_make(globals()" in src


# ---- C-ABI
def test_entry_point_declared_exported_and_checked():
    from pets_face_recognition_amd._hip.lib import LIB_PATH, parse_header
    protos = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    assert "pfr_pair_hist" in protos, "pfr_pair_hist not declared in include/pfr_hip.h"
    assert hasattr(dll, "pfr_pair_hist"), "pfr_pair_hist not exported by libpfr_hip.so"
    assert protos["pfr_pair_hist"][2] == ["a", "a_scale", "a_cls", "Na", "b", "b_scale", "b_cls", "Nb", "dtype", "D", "lo", "inv_w", "bins",
                                          "hist", "stream"]
    inc = open(os.path.join(os.path.dirname(LIB_PATH), "pfr_thunks_gen.inc")).read()
    assert '{"pfr_pair_hist", th_pfr_pair_hist}' in inc
    hdr = open(os.path.join(ROOT, "include", "pfr_hip.h")).read()
    assert "fminf(fmaxf(t, 0), bins - 1)" in hdr          # the bin rule is part of the header


def test_argument_checks_fail_before_any_launch():
    from pets_face_recognition_amd._hip import lib, PfrError
    # pointers are never dereferenced on the host: every call fails its geometry check first
    call = lambda dtype=1, D=64, lo=-1.0, inv_w=32.0, bins=64: lib.pfr_pair_hist(16, 0, 16, 8, 0, 0, 0, 0, dtype, D, lo, inv_w, bins, 16, 0)
    for kw in (dict(bins=0), dict(bins=8193), dict(dtype=3), dict(D=48), dict(dtype=0, D=48), dict(dtype=2, D=64), dict(dtype=2, D=1152),
               dict(inv_w=0.0), dict(inv_w=float("inf")), dict(lo=float("nan"))):
        with pytest.raises(PfrError):
            call(**kw)
