"""Host side of the DBSCAN clustering (no GPU): the plain-Python oracle (tests/dbscan_oracle.py) against scikit-learn, the CPU paths of
match.dbscan / match.neighbor_counts against the oracle, the identity with match.cluster at min_samples=1, ClusterStats(noise=-1) on a
hand count, the opt-in keys of the Controller, eval_fe.py's flag, and the C-ABI declarations."""
import math
import os
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_oracle as O
import dbscan_oracle as DO

from pets_face_recognition_amd import match
from pets_face_recognition_amd._hip import PfrError
from pets_face_recognition_amd.engine.metrics import ClusterStats

INF = float("inf")
MIN_SAMPLES = (1, 2, 3, 5, 8)


def _unit_scores(n, d, seed):
    """random unit rows and their fp32 score matrix as the CPU path computes it (one matmul of the normalised rows)"""
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(seed))
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return x, xn @ xn.t()


def _blobs(seed, n_centres=12, per=6, strays=20, d=16):
    """tight groups of 6 plus strays: every kind of node (core, border, noise) at thresholds around 0.8"""
    g = torch.Generator().manual_seed(seed)
    c = torch.nn.functional.normalize(torch.randn(n_centres, d, generator=g), dim=1)
    x = torch.cat([c.repeat_interleave(per, 0) + 0.18 * torch.randn(n_centres * per, d, generator=g), torch.randn(strays, d, generator=g)])
    return x[torch.randperm(x.shape[0], generator=g)]


# ---- the oracle against scikit-learn
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_against_sklearn(seed):
    cl = pytest.importorskip("sklearn.cluster")
    import numpy as np
    x = _blobs(seed)
    xn = torch.nn.functional.normalize(x, dim=1)
    S = xn @ xn.t()
    n = S.shape[0]
    seen = set()
    for thr in (0.7, 0.8, 0.9):
        adj = DO.adjacency(S, thr)
        dist = 1.0 - np.asarray(adj, dtype=np.float64)         # 0 between neighbours, 1 otherwise
        np.fill_diagonal(dist, 0.0)
        for ms in MIN_SAMPLES:
            deg, core, labels = DO.dbscan(S, thr, ms)
            sk = cl.DBSCAN(eps=0.5, min_samples=ms, metric="precomputed").fit(dist)
            assert sorted(sk.core_sample_indices_.tolist()) == [x_ for x_ in range(n) if core[x_]], (thr, ms)
            assert [l < 0 for l in sk.labels_.tolist()] == [l < 0 for l in labels], (thr, ms)            # the noise set
            # the partition of the core points: same label here <=> same label there
            cores = [x_ for x_ in range(n) if core[x_]]
            ours, theirs = {}, {}
            for x_ in cores:
                ours.setdefault(labels[x_], []).append(x_)
                theirs.setdefault(int(sk.labels_[x_]), []).append(x_)
            assert sorted(ours.values()) == sorted(theirs.values()), (thr, ms)
            assert all(lab == min(members) for lab, members in ours.items())                               # the smallest core index
            # a border point's label is the label of one of its qualifying core neighbours (which one is a rule of ours)
            for x_ in range(n):
                if not core[x_] and labels[x_] >= 0:
                    assert labels[x_] in {labels[c] for c in cores if adj[x_][c]}, (thr, ms, x_)
            seen.add(tuple(k > 0 for k in DO.kinds(core, labels)))
    assert (True, True, True, True) in seen                      # some grid point has core, border and noise nodes at once


def test_oracle_border_rule_by_hand():
    x, want = exact_tie_rows()
    S = x @ x.t()
    deg, core, labels = DO.dbscan(S, 8.0, 4)
    assert deg == [3, 4, 4, 4, 4, 4, 4, 3, 2, 2, 2] and core == want["core"] and labels == want["labels"]
    assert DO.kinds(core, labels) == (8, 3, 0, 2)
    assert DO.dbscan(S, 8.0, 6)[2] == [-1] * 11                    # nobody has five neighbours: all noise
    assert DO.dbscan(S, 8.0, 1)[2] == [0] * 11                     # everybody core: the borders chain the two cliques (single linkage)
    # signed zeros: cliques {0, 1, 2, 3} and {4, 5, 6, 7} (1 within, -1 across); node 8 scores -0.0 with node 1, +0.0 with node 4, -1 with
    # the rest; threshold 0.0: both zeros qualify, and they TIE after -0.0 -> +0.0, so the smaller index (node 1, cluster 0) wins
    n = 9
    Z = [[-1.0] * n for _ in range(n)]
    for lo in (0, 4):
        for i in range(lo, lo + 4):
            for j in range(i + 1, lo + 4):
                Z[i][j] = 1.0
    Z[1][8], Z[4][8] = -0.0, 0.0
    deg, core, labels = DO.dbscan(Z, 0.0, 4)
    assert deg == [3, 4, 3, 3, 4, 3, 3, 3, 2] and core == [True] * 8 + [False] and labels == [0] * 4 + [4] * 4 + [0]
    Z[1][8], Z[4][8] = -1e-30, 0.0                                  # a score really below: no longer adjacent to node 1
    assert DO.dbscan(Z, 0.0, 4)[0][8] == 1 and DO.dbscan(Z, 0.0, 4)[2][8] == 4       # one neighbour left, the core node 4


# ---- the CPU paths against the oracle
@pytest.mark.parametrize("n", [1, 2, 65, 130])
def test_cpu_dbscan_and_counts_equal_the_oracle(n):
    x, S = _unit_scores(n, 16, n)
    v = S[torch.ones(n, n, dtype=torch.bool).triu(1)].sort().values
    thrs = [0.0] if n < 2 else [float(v[int(q * (v.numel() - 1))]) for q in (0.5, 0.9, 0.97)]       # (scores themselves: equality qualifies)
    for thr in thrs + [-INF, INF]:
        cnt = match.neighbor_counts(x, thr)
        for ms in MIN_SAMPLES:
            deg, core, want = DO.dbscan(S, thr, ms)
            assert cnt.dtype == torch.int64 and cnt.tolist() == deg, (n, thr)
            labels, cmask = match.dbscan(x, thr, min_samples=ms, return_core=True)
            assert labels.dtype == torch.int64 and cmask.dtype == torch.bool
            assert cmask.tolist() == core and labels.tolist() == want, (n, thr, ms)
            assert torch.equal(match.dbscan(x, thr, min_samples=ms), labels)


def test_cpu_blobs_have_every_kind_of_node():
    x = _blobs(5)
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    S = xn @ xn.t()
    seen = set()
    for thr in (0.7, 0.8):
        for ms in (3, 5):
            deg, core, want = DO.dbscan(S, thr, ms)
            labels, cmask = match.dbscan(x, thr, min_samples=ms, return_core=True)
            assert labels.tolist() == want and cmask.tolist() == core
            seen.add(tuple(k > 0 for k in DO.kinds(core, want)))
    assert (True, True, True, True) in seen


def exact_tie_rows():
    """Rows with entries in {0, 4} (D = 64): every dot product is an exact small integer in fp32 and bf16, and in int8 every row
    quantises to {0, 127} with the SAME scale, so equal dot products are equal scores there too.  Two core cliques — A = {0, 1, 2, 3}
    share axis 0, B = {4, 5, 6, 7} share axis 1 (score 16 within, 0 across) — every core k with two private axes 2 + 2 k and 3 + 2 k, and
    three border nodes that touch single cores through those private axes (threshold 8, min_samples=4, i.e. 3 neighbours):
      8:  16 with node 5 (B) and 16 with node 2 (A)   -> equal scores to cores of two clusters: the smaller index, node 2 -> cluster 0
      9:  16 with node 1 (A) and 32 with node 6 (B)   -> the strictly higher score wins over the smaller index -> cluster 4
      10: 32 with node 3 (A) and 32 with node 4 (B)   -> equal: node 3 -> cluster 0"""
    x = torch.zeros(11, 64)
    x[0:4, 0] = 4.0
    x[4:8, 1] = 4.0
    for k in range(8):
        x[k, 2 + 2 * k] = x[k, 3 + 2 * k] = 4.0
    x[8, 2 + 2 * 5] = x[8, 2 + 2 * 2] = 4.0
    x[9, 2 + 2 * 1] = x[9, 2 + 2 * 6] = x[9, 3 + 2 * 6] = 4.0
    x[10, 2 + 2 * 3] = x[10, 3 + 2 * 3] = x[10, 2 + 2 * 4] = x[10, 3 + 2 * 4] = 4.0
    return x, {"labels": [0, 0, 0, 0, 4, 4, 4, 4, 0, 4, 0], "core": [True] * 8 + [False] * 3}


def test_cpu_border_ties_on_exact_scores():
    x, want = exact_tie_rows()
    labels, core = match.dbscan(x, 8.0, min_samples=4, normalize=False, return_core=True)
    assert labels.tolist() == want["labels"] and core.tolist() == want["core"]
    assert match.neighbor_counts(x, 8.0, normalize=False).tolist() == [3, 4, 4, 4, 4, 4, 4, 3, 2, 2, 2]
    # the same set in another order: the labels follow the indices (smallest core index, smallest tied neighbour)
    perm = torch.tensor([10, 4, 9, 0, 5, 8, 1, 6, 2, 7, 3])
    S = x[perm] @ x[perm].t()
    assert match.dbscan(x[perm], 8.0, min_samples=4, normalize=False).tolist() == DO.dbscan(S, 8.0, 4)[2]


# ---- identity and validation
@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_min_samples_one_equals_cluster(n):
    x = torch.randint(-2, 3, (n, 8), generator=torch.Generator().manual_seed(n)).float()
    for thr in (3.0, 9.0, -INF, INF):
        labels, core = match.dbscan(x, thr, min_samples=1, normalize=False, return_core=True)
        assert torch.equal(labels, match.cluster(x, thr, normalize=False)) and bool(core.all())
    y, _ = _unit_scores(n, 16, 7)
    assert torch.equal(match.dbscan(y, 0.3, min_samples=1), match.cluster(y, 0.3))


def test_nan_rows_are_noise():
    x = torch.randint(-2, 3, (40, 8), generator=torch.Generator().manual_seed(3)).float()
    x[7] = float("nan")
    assert match.neighbor_counts(x, -INF, normalize=False).tolist() == [38] * 7 + [0] + [38] * 32
    labels = match.dbscan(x, -INF, min_samples=2, normalize=False)
    assert labels[7] == -1 and (labels[:7] == 0).all() and (labels[8:] == 0).all()
    assert match.dbscan(x, -INF, min_samples=1, normalize=False)[7] == 7                 # a singleton cluster when everything is core
    assert (match.dbscan(x, float("nan"), min_samples=2, normalize=False) == -1).all()  # a NaN threshold: nothing qualifies
    assert (match.dbscan(x, INF, min_samples=2, normalize=False) == -1).all()


def test_argument_validation():
    x = torch.randn(10, 8, generator=torch.Generator().manual_seed(0))
    for bad in (0, -1, 2.0, "4", None, True):
        with pytest.raises(PfrError):
            match.dbscan(x, 0.5, min_samples=bad)
    with pytest.raises(PfrError):
        match.dbscan(x, 0.5, chunk=0)
    with pytest.raises(PfrError):
        match.neighbor_counts(x, 0.5, chunk=0)
    with pytest.raises(PfrError):
        match.dbscan(x[0], 0.5)
    with pytest.raises(PfrError):
        match.dbscan(x, 0.5, compute_dtype=torch.float16)
    with pytest.raises(PfrError):
        match.neighbor_counts(x, 0.5, compute_dtype=torch.float16)
    assert match.dbscan(x, 0.5, min_samples=1).tolist() == match.cluster(x, 0.5).tolist()
    assert "DBSCAN or Chinese whispers" not in match.cluster.__doc__ and "dbscan" in match.cluster.__doc__


# ---- ClusterStats(noise=...)
KEYS = ["pairwise_precision", "pairwise_recall", "pairwise_f", "bcubed_precision", "bcubed_recall", "bcubed_f", "clusters", "singletons"]


def test_cluster_stats_noise_against_a_hand_count():
    # clusters {0, 1, 2} (classes a a b) and {3} (class b); noise: items 4, 5 (class a) and 6 (class c)
    labels = torch.tensor([0, 0, 0, 3, -1, -1, -1])
    classes = torch.tensor([0, 0, 1, 1, 0, 0, 2])
    st = ClusterStats(labels, classes, noise=-1)
    m = st.metrics()
    assert list(m.keys()) == KEYS + ["noise"]
    assert st.noise == 3 and m["noise"] == 3 and m["clusters"] == 2 and m["singletons"] == 1
    # predicted pairs: C(3, 2) = 3 (the noise items predict none); TP = 1 (items 0, 1); true pairs: C(4, 2) + C(2, 2) + 0 = 7
    assert st.tp == 1 and st.cluster_pairs == 3 and st.class_pairs == 7
    assert m["pairwise_precision"] == 1 / 3 and m["pairwise_recall"] == 1 / 7
    # BCubed precision: items 0, 1: 2/3; item 2: 1/3; the four clusters of one: 1 -> (2/3 + 2/3 + 1/3 + 4) / 7
    assert abs(m["bcubed_precision"] - (5 / 3 + 4) / 7) < 1e-15
    # BCubed recall: class a (4 items): items 0, 1: 2/4; 4, 5: 1/4; class b (2): 1/2 each; class c: 1 -> (1 + 1/2 + 1 + 1) / 7
    assert abs(m["bcubed_recall"] - 3.5 / 7) < 1e-15
    # the same numbers as giving every noise item a label of its own by hand
    by_hand = ClusterStats(torch.tensor([0, 0, 0, 3, 100, 101, 102]), classes).metrics()
    for k in KEYS[:6]:
        assert m[k] == by_hand[k], k
    assert by_hand["clusters"] == 5 and by_hand["singletons"] == 4
    # noise=None: exactly what it was — the -1 items are one cluster of three
    plain = ClusterStats(labels, classes)
    assert plain.noise is None and list(plain.metrics().keys()) == KEYS
    O.assert_metrics_equal(plain.metrics(), O.metrics(labels.tolist(), classes.tolist()))
    assert plain.metrics()["clusters"] == 3 and plain.cluster_pairs == 6
    # a noise label that does not occur, and a set that is all noise
    m0 = ClusterStats(torch.tensor([0, 0, 5]), torch.tensor([1, 1, 2]), noise=-1).metrics()
    assert m0["noise"] == 0 and m0["clusters"] == 2 and {k: m0[k] for k in KEYS} == ClusterStats(torch.tensor([0, 0, 5]), torch.tensor([1, 1, 2])).metrics()
    ma = ClusterStats(torch.full((4,), -1), torch.tensor([0, 0, 1, 1]), noise=-1).metrics()
    assert ma["noise"] == 4 and ma["clusters"] == 0 and ma["singletons"] == 0 and math.isnan(ma["pairwise_precision"])
    assert ma["pairwise_recall"] == 0.0 and ma["bcubed_precision"] == 1.0 and ma["bcubed_recall"] == 0.5


# ---- Controller and eval_fe.py
def dbscan_keys(thrs):
    return [f"DBSCAN {name} thr={t}" for name in ("F", "precision", "recall", "BCubed F", "clusters", "noise") for t in thrs]


@pytest.mark.parametrize("method", ["_evaluate", "test_epoch_end"])
def test_controller_dbscan_keys_and_values_on_the_separated_set(method):
    from test_cluster_host import _controller, _cluster_keys, separated_set
    emb, classes = separated_set()
    base_c, batches, _, _ = _controller({"cluster": dict(thresholds=[0.9])}, emb, classes)
    base = getattr(base_c, method)([batches])["Val"]
    assert not any(k.startswith("DBSCAN") for k in base)                            # opt-in
    thrs = [0.9, "opt", 0.75]
    c, batches, _, _ = _controller({"cluster": dict(thresholds=[0.9]), "dbscan": dict(thresholds=thrs, min_samples=3)}, emb, classes)
    m = getattr(c, method)([batches])["Val"]
    assert list(m.keys()) == list(base.keys()) + dbscan_keys(thrs)                   # appended after the cluster keys
    assert list(base.keys())[-5:] == _cluster_keys([0.9])
    for k, v in base.items():
        assert m[k] == v or (v != v and m[k] != m[k]), k
    # classes of 3, tight and far apart: with min_samples=3 every item is core (two neighbours) and the classes are the clusters
    assert m["DBSCAN F thr=0.9"] == 1.0 and m["DBSCAN precision thr=0.9"] == 1.0 and m["DBSCAN recall thr=0.9"] == 1.0
    assert m["DBSCAN BCubed F thr=0.9"] == 1.0 and m["DBSCAN clusters thr=0.9"] == 20 and m["DBSCAN noise thr=0.9"] == 0
    # the values are ClusterStats(noise=-1) of match.dbscan at float32(2 t - 1) on the cosine; 'opt' is the run's own threshold
    from pets_face_recognition_amd.engine.metrics import PairStats
    opt = PairStats(*c._pair_scores(emb, c.config.pair_generator(0)[1])).opt_threshold()
    for t in thrs:
        sim = opt if t == "opt" else t
        st = ClusterStats(match.dbscan(emb, 2.0 * float(sim) - 1.0, min_samples=3), classes, noise=-1)
        p, r, f = st.pairwise()
        for key, want in ((f"DBSCAN F thr={t}", f), (f"DBSCAN precision thr={t}", p), (f"DBSCAN recall thr={t}", r),
                          (f"DBSCAN BCubed F thr={t}", st.bcubed()[2]), (f"DBSCAN clusters thr={t}", st.clusters),
                          (f"DBSCAN noise thr={t}", st.noise)):
            assert m[key] == want or (want != want and m[key] != m[key]), key
    # min_samples=4 (the default): nobody has three neighbours -> everything is noise, no cluster
    c4, batches, _, _ = _controller({"dbscan": dict(thresholds=[0.9])}, emb, classes)
    m4 = getattr(c4, method)([batches])["Val"]
    assert m4["DBSCAN noise thr=0.9"] == 60 and m4["DBSCAN clusters thr=0.9"] == 0 and m4["DBSCAN recall thr=0.9"] == 0.0
    assert math.isnan(m4["DBSCAN precision thr=0.9"])
    # an empty list opts in and adds nothing
    c0, batches, _, _ = _controller({"cluster": dict(thresholds=[0.9]), "dbscan": dict(thresholds=[])}, emb, classes)
    assert list(getattr(c0, method)([batches])["Val"].keys()) == list(base.keys())


def test_eval_fe_flag_reaches_the_config(monkeypatch):
    sys.path.insert(0, ROOT)
    import eval_fe
    seen = {}

    class FakeController:
        def __init__(self, config):
            seen["dbscan"] = config.get("dbscan")

    class FakeTrainer:
        def test(self, controller):
            return "tested"

    monkeypatch.setattr(eval_fe, "Controller", FakeController)
    monkeypatch.setattr(eval_fe, "configure_trainer", lambda *a, **k: FakeTrainer())
    with tempfile.TemporaryDirectory() as td:
        cfg = os.path.join(td, "cfg.py")
        open(cfg, "w").write("n_epochs = 1\ndevice = 'cpu'\n")
        assert eval_fe.main(["-c", cfg, "--dbscan", "4", "0.8", "opt", "0.95"]) == "tested"
        assert seen["dbscan"] == dict(thresholds=[0.8, "opt", 0.95], min_samples=4)
        assert eval_fe.main(["-c", cfg]) == "tested"
        assert seen["dbscan"] is None
        with pytest.raises(ValueError):
            eval_fe.main(["-c", cfg, "--dbscan", "4", "high"])
        with pytest.raises(SystemExit):
            eval_fe.main(["-c", cfg, "--dbscan", "4"])


def test_dbscan_config_sets_the_key():
    src = open(os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic", "fe_r18_mi355x_dbscan.py")).read()
    assert "dbscan = dict(thresholds=" in src and "min_samples=" in src and "_make(globals()" in src


# ---- C-ABI
def test_header_declares_the_entry_points():
    from pets_face_recognition_amd._hip.lib import LIB_PATH, parse_header
    protos = parse_header()
    assert {"pfr_neighbor_count", "pfr_dbscan_link", "pfr_dbscan_labels"} <= set(protos)
    operands = ["a", "a_scale", "Na", "a_off", "b", "b_scale", "Nb", "b_off", "dtype", "D", "thr"]
    assert protos["pfr_neighbor_count"][2] == operands + ["deg", "n_nodes", "stream"]
    assert protos["pfr_dbscan_link"][2] == operands + ["deg", "min_neighbors", "parent", "best", "n_nodes", "status", "stream"]
    assert protos["pfr_dbscan_labels"][2] == ["parent", "deg", "best", "min_neighbors", "n_nodes", "labels", "stream"]
    inc = open(os.path.join(os.path.dirname(LIB_PATH), "pfr_thunks_gen.inc")).read()
    for name in ("pfr_neighbor_count", "pfr_dbscan_link", "pfr_dbscan_labels"):
        assert f'{{"{name}", th_{name}}}' in inc
    hdr = open(os.path.join(ROOT, "include", "pfr_hip.h")).read()
    assert "min_neighbors = min_samples - 1" in hdr and "SMALLEST\n *       CORE INDEX" in hdr and "0xffffffff - c" in hdr


def test_argument_checks_fail_before_any_launch():
    from pets_face_recognition_amd._hip import lib
    # pointers are never dereferenced on the host: every call fails a geometry check first
    def count(Na=8, a_off=0, b=0, Nb=0, b_off=0, dtype=1, D=64, n_nodes=64):
        return lib.pfr_neighbor_count(16, 0, Na, a_off, b, 0, Nb, b_off, dtype, D, 0.5, 16, n_nodes, 0)

    def link(Na=8, a_off=0, b=0, Nb=0, b_off=0, dtype=1, D=64, n_nodes=64, mn=2):
        return lib.pfr_dbscan_link(16, 0, Na, a_off, b, 0, Nb, b_off, dtype, D, 0.5, 16, mn, 16, 16, n_nodes, 16, 0)
    for kw in (dict(dtype=3), dict(D=48), dict(dtype=0, D=48), dict(dtype=2, D=64), dict(Na=-1), dict(b=16, Nb=-1), dict(a_off=-1),
               dict(b=16, Nb=8, b_off=-1), dict(n_nodes=-1), dict(n_nodes=7), dict(a_off=57), dict(b=16, Nb=8, b_off=57),
               dict(a_off=2 ** 31 - 8, n_nodes=2 ** 31 - 1), dict(b=16, Nb=8, b_off=2 ** 31 - 8, n_nodes=2 ** 31 - 1)):
        with pytest.raises(PfrError):
            count(**kw)
        with pytest.raises(PfrError):
            link(**kw)
    with pytest.raises(PfrError):
        link(mn=-1)
    with pytest.raises(PfrError):
        lib.pfr_dbscan_labels(16, 16, 16, 2, -1, 16, 0)
    with pytest.raises(PfrError):
        lib.pfr_dbscan_labels(16, 16, 16, -1, 8, 16, 0)
    # nothing to do: no pointer is looked at
    assert count(Na=0) == 0 and count(Na=1) == 0 and count(b=16, Nb=0) == 0
    assert link(Na=0) == 0 and link(Na=1) == 0 and link(b=16, Nb=0) == 0
    assert lib.pfr_dbscan_labels(0, 0, 0, 0, 0, 0, 0) == 0
