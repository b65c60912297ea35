"""Host side of the threshold clustering (no GPU): engine.metrics.ClusterStats / match.cluster_metrics on hand-worked cases and against the
dense oracle (tests/cluster_oracle.py), the CPU paths of match.pairs_above / match.cluster against brute force on integer-valued rows
(exact scores), the opt-in keys of the Controller, eval_fe.py's flag, and the C-ABI declarations."""
import math
import os
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_oracle as O

from pets_face_recognition_amd import match
from pets_face_recognition_amd._hip import PfrError
from pets_face_recognition_amd.engine.metrics import ClusterStats, cluster_metrics

INF = float("inf")
KEYS = ["pairwise_precision", "pairwise_recall", "pairwise_f", "bcubed_precision", "bcubed_recall", "bcubed_f", "clusters", "singletons"]


# ---- metrics
def test_metrics_perfect_clustering():
    m = match.cluster_metrics(torch.tensor([0, 0, 0, 3, 3]), torch.tensor([7, 7, 7, 2, 2]))
    assert list(m.keys()) == KEYS
    assert all(m[k] == 1.0 for k in KEYS[:6]) and m["clusters"] == 2 and m["singletons"] == 0


def test_metrics_everything_in_one_cluster():
    # classes of 3 and 2 in one cluster of 5: TP = 3 + 1 = 4 of 10 predicted pairs, every true pair found
    m = match.cluster_metrics(torch.zeros(5, dtype=torch.long), torch.tensor([0, 0, 0, 1, 1]))
    assert m["pairwise_precision"] == 0.4 and m["pairwise_recall"] == 1.0 and abs(m["pairwise_f"] - 0.8 / 1.4) < 1e-15
    # BCubed precision = (3 * 3/5 + 2 * 2/5) / 5 = 13 / 25, recall = 1
    assert abs(m["bcubed_precision"] - 0.52) < 1e-15 and m["bcubed_recall"] == 1.0 and abs(m["bcubed_f"] - 1.04 / 1.52) < 1e-15
    assert m["clusters"] == 1 and m["singletons"] == 0


def test_metrics_all_singletons():
    m = match.cluster_metrics(torch.arange(5), torch.tensor([0, 0, 0, 1, 1]))
    # no predicted pair: precision has nothing to measure; none of the 3 + 1 true pairs is found
    assert math.isnan(m["pairwise_precision"]) and m["pairwise_recall"] == 0.0 and math.isnan(m["pairwise_f"])
    # every item is alone and pure: precision 1; recall = (3 * 1/3 + 2 * 1/2) / 5 = 2 / 5
    assert m["bcubed_precision"] == 1.0 and abs(m["bcubed_recall"] - 0.4) < 1e-15 and abs(m["bcubed_f"] - 0.8 / 1.4) < 1e-15
    assert m["clusters"] == 5 and m["singletons"] == 5
    # singletons that are right: one item per class — no pair on either side
    m = match.cluster_metrics(torch.arange(4), torch.arange(4))
    assert math.isnan(m["pairwise_precision"]) and math.isnan(m["pairwise_recall"]) and math.isnan(m["pairwise_f"])
    assert m["bcubed_precision"] == 1.0 and m["bcubed_recall"] == 1.0 and m["bcubed_f"] == 1.0


def test_metrics_textbook_example():
    # three clusters of 17 items (x, o, d): {5 x, 1 o}, {1 x, 4 o, 1 d}, {2 x, 3 d} — the worked example of the IR textbooks:
    # TP = 10 + 6 + 1 + 3 = 20, predicted pairs 15 + 15 + 10 = 40, true pairs C(8,2) + C(5,2) + C(4,2) = 44
    labels = [0] * 6 + [1] * 6 + [2] * 5
    classes = [0] * 5 + [1] + [0] + [1] * 4 + [2] + [0] * 2 + [2] * 3
    m = match.cluster_metrics(torch.tensor(labels), torch.tensor(classes))
    assert m["pairwise_precision"] == 0.5 and abs(m["pairwise_recall"] - 20 / 44) < 1e-15
    assert abs(m["pairwise_f"] - 2 * 0.5 * (20 / 44) / (0.5 + 20 / 44)) < 1e-15
    # BCubed precision = (26/6 + 18/6 + 13/5) / 17, recall = (30/8 + 17/5 + 10/4) / 17
    assert abs(m["bcubed_precision"] - (26 / 6 + 3 + 2.6) / 17) < 1e-14 and abs(m["bcubed_recall"] - 9.65 / 17) < 1e-14
    assert m["clusters"] == 3 and m["singletons"] == 0
    O.assert_metrics_equal(m, O.metrics(labels, classes))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_metrics_random_labelings_equal_the_dense_oracle(seed):
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, 40, (500,), generator=g) * 3 - 7          # (arbitrary ids, negative included)
    classes = torch.randint(0, 30, (500,), generator=g)
    st = ClusterStats(labels, classes)
    O.assert_metrics_equal(st.metrics(), O.metrics(labels.tolist(), classes.tolist()))
    assert cluster_metrics(labels, classes) == st.metrics()
    p, r, f = st.pairwise()
    assert 0.0 < p < 1.0 and 0.0 < r < 1.0 and min(p, r) <= f <= max(p, r)
    with pytest.raises(ValueError):
        ClusterStats(labels, classes[:-1])


# ---- CPU paths against brute force
def _int_rows(n, d, seed):
    """integer-valued rows in [-2, 2]: every dot product is exact in fp32 and many of them are equal"""
    return torch.randint(-2, 3, (n, d), generator=torch.Generator().manual_seed(seed)).float()


def _brute(a, b, thr):
    sym = b is None
    bb = a if sym else b
    out = []
    for i in range(a.shape[0]):
        for j in range(i + 1 if sym else 0, bb.shape[0]):
            s = float((a[i].double() * bb[j].double()).sum())
            if s >= thr:
                out.append((i, j, s))
    return out


def _as_list(res):
    i, j, s = res
    assert i.dtype == torch.int64 and j.dtype == torch.int64 and s.dtype == torch.float32
    return list(zip(i.tolist(), j.tolist(), s.tolist()))


@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_cpu_pairs_and_labels_equal_brute_force(n):
    x = _int_rows(n, 8, n)
    for thr in (3.0, 9.0, -INF, INF):
        want = _brute(x, None, thr)
        assert _as_list(match.pairs_above(x, thr, normalize=False)) == want, (n, thr)      # (sorted by (i, j) like the double loop)
        labels = match.cluster(x, thr, normalize=False)
        assert labels.dtype == torch.int64 and labels.tolist() == O.components(n, [(i, j) for i, j, _ in want]), (n, thr)
    assert len(_brute(x, None, -INF)) == n * (n - 1) // 2 and _brute(x, None, INF) == []


def test_cpu_two_set_mode():
    a, b = _int_rows(70, 8, 1), _int_rows(130, 8, 2)
    for thr in (4.0, -INF, INF):
        assert _as_list(match.pairs_above(a, thr, emb_b=b, normalize=False)) == _brute(a, b, thr)
    assert len(match.pairs_above(a, -INF, emb_b=b, normalize=False)[0]) == 70 * 130


def test_cpu_nan_row_yields_no_pair():
    x = _int_rows(40, 8, 3)
    x[7] = float("nan")
    i, j, s = match.pairs_above(x, -INF, normalize=False)
    assert len(i) == 39 * 38 // 2 and 7 not in i.tolist() and 7 not in j.tolist() and not bool(torch.isnan(s).any())
    labels = match.cluster(x, -INF, normalize=False)
    assert labels[7] == 7 and (labels[:7] == 0).all() and (labels[8:] == 0).all()


def test_cpu_threshold_is_on_the_normalised_dot_product():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(50, 16, generator=g)
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    s = xn @ xn.t()
    i, j, sc = match.pairs_above(x, 0.2)
    want = O.edges_from_scores(s, 0.2, True)
    assert list(zip(i.tolist(), j.tolist())) == want and torch.equal(sc, s[i, j])
    assert match.cluster(x, 0.2).tolist() == O.components(50, want)


def test_cpu_max_pairs_and_argument_errors():
    x = _int_rows(65, 8, 5)
    n = len(_brute(x, None, 3.0))
    assert len(match.pairs_above(x, 3.0, normalize=False, max_pairs=n)[0]) == n
    with pytest.raises(PfrError, match=str(n)):
        match.pairs_above(x, 3.0, normalize=False, max_pairs=n - 1)
    with pytest.raises(PfrError):
        match.pairs_above(x, 3.0, max_pairs=-1)
    with pytest.raises(PfrError):
        match.pairs_above(x, 3.0, emb_b=x[:, :4])
    with pytest.raises(PfrError):
        match.pairs_above(x, 3.0, compute_dtype=torch.float16)
    with pytest.raises(PfrError):
        match.cluster(x, 3.0, chunk=0)
    with pytest.raises(PfrError):
        match.cluster(x[0], 3.0)


# ---- Controller and eval_fe.py
def _controller(extra, emb=None, classes=None):
    """a Controller over a fe_r18_cpu-style config (thrs, k, far_thr, frr_thr, the default cosine similarity) on fixed embeddings"""
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


def _cluster_keys(thrs):
    return [f"{name} thr={t}" for name in ("Cluster F", "Cluster precision", "Cluster recall", "Cluster BCubed F", "Clusters") for t in thrs]


@pytest.mark.parametrize("method", ["_evaluate", "test_epoch_end"])
def test_controller_cluster_is_opt_in_and_its_keys_come_last(method):
    from pets_face_recognition_amd.engine.metrics import PairStats
    c0, batches, emb, classes = _controller({})
    base = getattr(c0, method)([batches])["Val"]
    assert not any(k.startswith("Cluster") for k in base)
    want_base = (["ROC AUC", "AveragePrecision", "Accuracy", "Opt thr", "Accuracy thr=0.6", "Accuracy thr=0.8", "Precision thr=0.6",
                  "Precision thr=0.8", "Recall thr=0.6", "Recall thr=0.8", "Recall@K=1", "Recall@K=5", "TAR@FAR=0.1", "TH@FAR=0.1",
                  "TAR@FAR=0.05", "TH@FAR=0.05", "TRR@FRR=0.1", "TH@FRR=0.1"] if method == "_evaluate"
                 else ["ROC AUC", "Accuracy", "Recall@K=10", "Recall@K=100"])
    assert list(base.keys()) == want_base                       # key for key what it is without the feature
    thrs = [0.8, "opt", 0.95]
    c1, batches, _, _ = _controller({"cluster": dict(thresholds=thrs), "retrieval": dict(ks=[1])})
    c2, _, _, _ = _controller({"retrieval": dict(ks=[1])})
    m = getattr(c1, method)([batches])["Val"]
    before = getattr(c2, method)([batches])["Val"]
    assert list(m.keys()) == list(before.keys()) + _cluster_keys(thrs)          # after every existing key, opt-in ones included
    for k, v in before.items():
        assert m[k] == v or (v != v and m[k] != m[k]), k
    # the values: clustering at float32(2 t - 1) on the cosine, scored against the classes
    ci = c1._pair_scores(emb, c1.config.pair_generator(0)[1])
    opt = PairStats(*ci).opt_threshold()
    if method == "_evaluate":
        assert m["Opt thr"] == opt                               # 'opt' resolves to the run's own Opt thr
    for t in thrs:
        sim = opt if t == "opt" else t
        st = ClusterStats(match.cluster(emb, 2.0 * float(sim) - 1.0), classes)
        assert m[f"Cluster F thr={t}"] == st.pairwise()[2] or math.isnan(st.pairwise()[2])
        assert m[f"Cluster precision thr={t}"] == st.pairwise()[0] or math.isnan(st.pairwise()[0])
        assert m[f"Cluster recall thr={t}"] == st.pairwise()[1]
        assert m[f"Cluster BCubed F thr={t}"] == st.bcubed()[2]
        assert m[f"Clusters thr={t}"] == st.clusters and 1 <= st.clusters <= 60
    assert m["Clusters thr=0.8"] <= m["Clusters thr=0.95"]       # a higher threshold never merges more
    # an empty list opts in and adds nothing
    c3, batches, _, _ = _controller({"cluster": dict(thresholds=[])})
    assert list(getattr(c3, method)([batches])["Val"].keys()) == list(base.keys())


def separated_set():
    """60 items in 20 tight, well separated classes of 3 (within-class cosine ~ 1, between classes far below 0.8)"""
    g = torch.Generator().manual_seed(11)
    classes = torch.arange(60) // 3
    centres = torch.nn.functional.normalize(torch.randn(20, 64, generator=g), dim=1)
    return centres[classes] + 0.01 * torch.randn(60, 64, generator=g), classes


@pytest.mark.parametrize("method", ["_evaluate", "test_epoch_end"])
def test_controller_separated_clusters_are_recovered(method):
    emb, classes = separated_set()
    c, batches, _, _ = _controller({"cluster": dict(thresholds=[0.9])}, emb, classes)
    m = getattr(c, method)([batches])["Val"]
    assert m["Cluster F thr=0.9"] == 1.0 and m["Cluster BCubed F thr=0.9"] == 1.0 and m["Clusters thr=0.9"] == 20


def test_eval_fe_flag_reaches_the_config(monkeypatch):
    sys.path.insert(0, ROOT)
    import eval_fe
    seen = {}

    class FakeController:
        def __init__(self, config):
            seen["cluster"] = config.get("cluster")

    class FakeTrainer:
        def test(self, controller):
            return "tested"

    monkeypatch.setattr(eval_fe, "Controller", FakeController)
    monkeypatch.setattr(eval_fe, "configure_trainer", lambda *a, **k: FakeTrainer())
    with tempfile.TemporaryDirectory() as td:
        cfg = os.path.join(td, "cfg.py")
        open(cfg, "w").write("n_epochs = 1\ndevice = 'cpu'\n")
        assert eval_fe.main(["-c", cfg, "--cluster", "0.8", "opt", "0.95"]) == "tested"
        assert seen["cluster"] == dict(thresholds=[0.8, "opt", 0.95])
        assert eval_fe.main(["-c", cfg]) == "tested"
        assert seen["cluster"] is None
        with pytest.raises(ValueError):
            eval_fe.main(["-c", cfg, "--cluster", "high"])


def test_cluster_config_sets_the_key():
    src = open(os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic", "fe_r18_mi355x_cluster.py")).read()
    assert "cluster = dict(thresholds=" in src and "_make(globals()" in src


# ---- C-ABI
def test_header_declares_the_entry_points():
    from pets_face_recognition_amd._hip.lib import LIB_PATH, parse_header
    protos = parse_header()
    assert {"pfr_pairs_above", "pfr_cc_union", "pfr_cc_flatten"} <= set(protos)
    assert protos["pfr_pairs_above"][2] == ["a", "a_scale", "Na", "a_off", "b", "b_scale", "Nb", "b_off", "dtype", "D", "thr", "edge_i",
                                            "edge_j", "edge_s", "cap", "count", "parent", "n_nodes", "status", "stream"]
    assert protos["pfr_cc_union"][2] == ["parent", "n_nodes", "edge_i", "edge_j", "E", "status", "stream"]
    assert protos["pfr_cc_flatten"][2] == ["parent", "n_nodes", "labels", "stream"]
    inc = open(os.path.join(os.path.dirname(LIB_PATH), "pfr_thunks_gen.inc")).read()
    for name in ("pfr_pairs_above", "pfr_cc_union", "pfr_cc_flatten"):
        assert f'{{"{name}", th_{name}}}' in inc
    hdr = open(os.path.join(ROOT, "include", "pfr_hip.h")).read()
    assert "6 * n_nodes + 64" in hdr and "MAY ALIAS" in hdr          # the loop cap and the aliasing rule are part of the header


def test_argument_checks_fail_before_any_launch():
    from pets_face_recognition_amd._hip import lib
    # pointers are never dereferenced on the host: every call fails a geometry check first
    def call(Na=8, a_off=0, b=0, Nb=0, b_off=0, dtype=1, D=64, edge_i=16, edge_j=16, cap=4, count=16, parent=0, n_nodes=0, status=0):
        return lib.pfr_pairs_above(16, 0, Na, a_off, b, 0, Nb, b_off, dtype, D, 0.5, edge_i, edge_j, 0, cap, count, parent, n_nodes, status, 0)
    big = 2 ** 31 - 1
    for kw in (dict(dtype=3), dict(D=48), dict(dtype=0, D=48), dict(dtype=2, D=64), dict(dtype=2, D=1152), dict(Na=-1),
               dict(b=16, Nb=-1), dict(cap=-1), dict(a_off=-1), dict(b=16, Nb=8, b_off=-1), dict(a_off=big - 7),
               dict(b=16, Nb=8, b_off=big - 7), dict(edge_i=0, edge_j=0, count=0), dict(edge_j=0), dict(count=0),
               dict(edge_i=0, edge_j=0, count=0, parent=16, n_nodes=8, status=0), dict(parent=16, n_nodes=-1, status=16)):
        with pytest.raises(PfrError):
            call(**kw)
    with pytest.raises(PfrError):
        lib.pfr_cc_union(16, -1, 16, 16, 4, 16, 0)
    with pytest.raises(PfrError):
        lib.pfr_cc_union(16, 8, 16, 16, -4, 16, 0)
    with pytest.raises(PfrError):
        lib.pfr_cc_flatten(16, -1, 16, 0)
    # nothing to do: no pointer is looked at
    assert lib.pfr_pairs_above(0, 0, 0, 0, 0, 0, 0, 0, 1, 64, 0.5, 16, 16, 0, 4, 16, 0, 0, 0, 0) == 0
    assert lib.pfr_pairs_above(0, 0, 1, 0, 0, 0, 0, 0, 1, 64, 0.5, 16, 16, 0, 4, 16, 0, 0, 0, 0) == 0
    assert lib.pfr_cc_union(0, 8, 0, 0, 0, 0, 0) == 0 and lib.pfr_cc_flatten(0, 0, 0, 0) == 0
