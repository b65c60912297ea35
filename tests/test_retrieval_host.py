"""Exact retrieval ranks and mAP / CMC / mINP on the host: the CPU path of match.positive_ranks / retrieval_metrics against the brute-force
oracle (tests/retrieval_oracle.py) on tie-heavy integer rows, the hand-computed and duplicate-row cases of the tie rule, the IEEE rule
for NaN rows, engine.metrics.RankStats, and the opt-in keys of the Controller and of eval_fe.py."""
import math
import os
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retrieval_oracle as O

from pets_face_recognition_amd import match
from pets_face_recognition_amd._hip import PfrError
from pets_face_recognition_amd.engine.metrics import RankStats, rank_metrics

KS = (1, 5, 10)


def _int_rows(n, d, seed):
    """integer-valued rows in [-2, 2]: every dot product is exact in fp32 and many of them are equal"""
    return torch.randint(-2, 3, (n, d), generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("layout", ["random7", "equal", "distinct"])
@pytest.mark.parametrize("n", [2, 5, 64, 130])
def test_cpu_ranks_and_metrics_equal_the_oracle(n, layout):
    emb, cls = _int_rows(n, 8, n), O.class_layout(layout, n, seed=n)
    ranks, npos = match.positive_ranks(emb, cls, normalize=False)
    assert ranks.dtype == torch.int32 and npos.dtype == torch.int32 and ranks.shape[0] == n
    want = O.ranks_from_scores(emb @ emb.t(), cls, cls, True)
    assert O.as_lists(ranks, npos) == want
    got = match.retrieval_metrics(emb, cls, ks=KS, normalize=False)
    O.assert_metrics_equal(got, O.metrics(want, KS))
    if layout == "distinct":
        assert got["queries"] == 0 and math.isnan(got["mAP"]) and math.isnan(got["CMC@K=1"]) and ranks.shape[1] == 0
    if layout == "equal":
        # every other item is a positive: the ranks are 1 .. n - 1 whatever the scores
        assert all(r == list(range(1, n)) for r in want) and got["mAP"] == 1.0


def test_cpu_query_gallery_mode_equals_the_oracle():
    q, g = _int_rows(7, 8, 1), _int_rows(40, 8, 2)
    cq, cg = O.class_layout("random7", 7, 3), O.class_layout("random7", 40, 4)
    g[5] = q[2]                                      # a gallery copy of a query is NOT excluded in this mode
    ranks, npos = match.positive_ranks(q, cq, g, cg, normalize=False)
    want = O.ranks_from_scores(q @ g.t(), cq, cg, False)
    assert O.as_lists(ranks, npos) == want
    O.assert_metrics_equal(match.retrieval_metrics(q, cq, g, cg, ks=KS, normalize=False), O.metrics(want, KS))


def test_hand_computed_case():
    # one query against nine items whose scores are 9, 8, ..., 1: its positives sit at ranks 1, 3 and 6
    q = torch.tensor([[1.0, 0.0]])
    g = torch.stack([torch.tensor([float(9 - j), 0.0]) for j in range(9)])
    cg = torch.tensor([0, 1, 0, 1, 1, 0, 1, 1, 1])
    ranks, npos = match.positive_ranks(q, torch.tensor([0]), g, cg, normalize=False)
    assert ranks.tolist() == [[1, 3, 6]] and npos.tolist() == [3]
    m = match.retrieval_metrics(q, torch.tensor([0]), g, cg, ks=(1, 2, 3), normalize=False)
    assert abs(m["mAP"] - (1 / 1 + 2 / 3 + 3 / 6) / 3) < 1e-15 and m["mINP"] == 3 / 6
    assert m["CMC@K=1"] == 1.0 and m["mean_first_rank"] == 1.0 and m["queries"] == 1


def test_duplicate_rows_take_the_order_of_their_indices():
    u = torch.tensor([1.0, 0.0, 0.0])
    lo = torch.tensor([0.0, 1.0, 0.0])
    # query 0; items 1..5 all score 1.0 with it: impostor (1), positive (2), positive (3), impostor (4); item 5 scores 0
    emb = torch.stack([u, u, u, u, u, lo])
    cls = torch.tensor([0, 1, 0, 0, 2, 3])
    ranks, npos = match.positive_ranks(emb, cls, normalize=False)
    # the identical impostor with the lower index (1) precedes both positives, the one with the higher index (4) neither; the two
    # identical positives take consecutive ranks, lower index first
    assert ranks[0].tolist() == [2, 3] and npos[0] == 2
    # seen from query 2 (positives 0 and 3): 0 and the impostor 1 come before 3
    assert ranks[2].tolist() == [1, 3]
    want = O.ranks_from_scores(emb @ emb.t(), cls, cls, True)
    assert O.as_lists(ranks, npos) == want


def test_nan_row_follows_the_ieee_rule():
    emb = _int_rows(6, 4, 5)
    emb[:, 0] = 3.0                                  # (no zero rows)
    cls = torch.tensor([0, 0, 0, 1, 1, 1])
    clean_r, _ = match.positive_ranks(emb, cls, normalize=False)
    emb[4] = float("nan")
    ranks, npos = match.positive_ranks(emb, cls, normalize=False)
    # a NaN score precedes nothing: queries 0..2 (no NaN positive) rank their positives among 4 items instead of 5 — every rank is the
    # clean rank minus one when item 4 preceded it, and never larger
    assert bool((ranks[:3] <= clean_r[:3]).all()) and bool((ranks[:3] >= clean_r[:3] - 1).all())
    # nothing precedes a NaN threshold: for the queries 3 and 5 the NaN positive counts nothing and so has rank 1
    assert ranks[3, 0] == 1 and ranks[5, 0] == 1
    # the NaN query: every score of its row is NaN, nothing precedes anything
    assert ranks[4].tolist() == [1, 1] and npos.tolist() == [2] * 6


def test_rank_stats_definitions_and_errors():
    ranks = torch.tensor([[1, 3, 6], [2, 0, 0], [0, 0, 0]], dtype=torch.int32)
    npos = torch.tensor([3, 1, 0], dtype=torch.int32)
    rs = RankStats(ranks, npos)
    assert rs.queries == 2
    assert abs(rs.mean_ap() - ((1 + 2 / 3 + 3 / 6) / 3 + 1 / 2) / 2) < 1e-15
    assert abs(rs.mean_inp() - (3 / 6 + 1 / 2) / 2) < 1e-15
    assert rs.cmc(1) == 0.5 and rs.cmc(2) == 1.0 and rs.mean_first_rank() == 1.5
    assert list(rank_metrics(ranks, npos, (1, 2)).keys()) == ["mAP", "mINP", "CMC@K=1", "CMC@K=2", "mean_first_rank", "queries"]
    empty = rank_metrics(torch.zeros((3, 0), dtype=torch.int32), torch.zeros(3, dtype=torch.int32))
    assert empty["queries"] == 0 and all(math.isnan(v) for k, v in empty.items() if k != "queries")
    with pytest.raises(ValueError):
        RankStats(ranks, torch.tensor([4, 1, 0]))
    with pytest.raises(ValueError):
        RankStats(torch.tensor([[0, 1]]), torch.tensor([2]))


def test_argument_errors():
    emb, cls = _int_rows(6, 8, 0), torch.arange(6)
    with pytest.raises(PfrError):
        match.positive_ranks(emb, cls[:5])
    with pytest.raises(PfrError):
        match.positive_ranks(emb, cls, emb_b=emb)
    with pytest.raises(PfrError):
        match.positive_ranks(emb, cls, emb[:, :4], cls)
    with pytest.raises(PfrError):
        match.positive_ranks(emb, cls, compute_dtype=torch.float16)
    with pytest.raises(PfrError):
        match.retrieval_metrics(emb, cls, ks=(0, 1))


# ---- Controller and eval_fe.py
def _controller(extra, emb=None, classes=None):
    from pets_face_recognition_amd.engine.controller import Controller
    g = torch.Generator().manual_seed(3)
    N = 60
    if emb is None:
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


@pytest.mark.parametrize("method", ["_evaluate", "test_epoch_end"])
def test_controller_retrieval_is_opt_in(method):
    c0, batches, emb, classes = _controller({})
    base = getattr(c0, method)([batches])["Val"]
    new = ["mAP", "mINP", "CMC@K=1", "CMC@K=3", "Mean first rank"]
    assert not any(k in new or k.startswith("CMC") for k in base)
    c1, batches, _, _ = _controller({"retrieval": dict(ks=[1, 3])})
    m = getattr(c1, method)([batches])["Val"]
    assert list(m.keys()) == list(base.keys()) + new
    for k, v in base.items():                     # the existing metrics do not move
        assert m[k] == v or (v != v and m[k] != m[k]), k
    want = match.retrieval_metrics(emb, classes, ks=(1, 3))
    assert m["mAP"] == want["mAP"] and m["mINP"] == want["mINP"] and m["CMC@K=3"] == want["CMC@K=3"]
    assert m["Mean first rank"] == want["mean_first_rank"]
    oracle = O.metrics(O.ranks_from_scores(torch.nn.functional.normalize(emb) @ torch.nn.functional.normalize(emb).t(), classes, classes,
                                           True), (1, 3))
    assert abs(m["mAP"] - oracle["mAP"]) < 1e-3   # (normalisation rounding may swap near-ties; the exact checks are above)


@pytest.mark.parametrize("method", ["_evaluate", "test_epoch_end"])
def test_controller_separated_clusters_are_perfect(method):
    g = torch.Generator().manual_seed(11)
    classes = torch.arange(60) // 3
    centres = torch.nn.functional.normalize(torch.randn(20, 64, generator=g), dim=1)
    emb = centres[classes] + 0.01 * torch.randn(60, 64, generator=g)
    c, batches, _, _ = _controller({"retrieval": dict(ks=[1, 5, 10])}, emb, classes)
    m = getattr(c, method)([batches])["Val"]
    assert m["mAP"] == 1.0 and m["CMC@K=1"] == 1.0 and m["mINP"] == 1.0 and m["Mean first rank"] == 1.0


def test_eval_fe_flag_reaches_the_config(monkeypatch):
    sys.path.insert(0, ROOT)
    import eval_fe
    seen = {}

    class FakeController:
        def __init__(self, config):
            seen["retrieval"] = config.get("retrieval")

    class FakeTrainer:
        def test(self, controller):
            return "tested"

    monkeypatch.setattr(eval_fe, "Controller", FakeController)
    monkeypatch.setattr(eval_fe, "configure_trainer", lambda *a, **k: FakeTrainer())
    with tempfile.TemporaryDirectory() as td:
        cfg = os.path.join(td, "cfg.py")
        open(cfg, "w").write("n_epochs = 1\ndevice = 'cpu'\n")
        assert eval_fe.main(["-c", cfg, "--retrieval", "1", "20"]) == "tested"
        assert seen["retrieval"] == dict(ks=[1, 20])
        assert eval_fe.main(["-c", cfg, "--retrieval"]) == "tested"
        assert seen["retrieval"] == dict(ks=[1, 5, 10])
        assert eval_fe.main(["-c", cfg]) == "tested"
        assert seen["retrieval"] is None


def test_retrieval_config_sets_the_key():
    src = open(os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic", "fe_r18_mi355x_retrieval.py")).read()
    assert "retrieval = dict(ks=" in src and "_make(globals()" in src


def test_header_declares_the_entry_points():
    from pets_face_recognition_amd._hip.lib import parse_header
    protos = parse_header()
    assert {"pfr_rank_count", "pfr_pair_scores_gather", "pfr_rank_count_max_thr"} <= set(protos)
    assert protos["pfr_rank_count"][2] == ["a", "a_scale", "Na", "b", "b_scale", "b_id", "Nb", "dtype", "D", "excl", "thr_val", "thr_id",
                                           "thr_cnt", "ld", "cnt", "stream"]
    assert match.rank_count_max_thr() >= 16
