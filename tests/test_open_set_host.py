"""Host side of the open-set identification (no GPU): the CPU path of match.class_extremes against the plain-Python oracle
(tests/open_set_oracle.py), the oracle's torch form against its loop form, engine.metrics.OpenSetStats against a brute-force loop on
hand-made vectors, match.label_suspects, the opt-in keys of the Controller, eval_fe.py's flag, the config and the C-ABI declarations.
Everything is exact: rows are integer valued, so fp32 dot products carry no rounding."""
import math
import os
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import open_set_oracle as OO

from pets_face_recognition_amd import match
from pets_face_recognition_amd._hip import PfrError
from pets_face_recognition_amd.engine.metrics import OpenSetStats

INF = float("inf")
NAN = float("nan")


def int_rows(n, d, seed, dup=True, nan_row=None):
    """integer-valued rows in -2 .. 2 (exact fp32 dots, many tied scores, zero dots of both signs of the factors); with `dup` rows 3 and
    n - 1 repeat row 0 (equal scores against everything: the tie rule decides); `nan_row` is all NaN"""
    x = torch.randint(-2, 3, (n, d), generator=torch.Generator().manual_seed(seed)).float()
    if dup and n > 4:
        x[3] = x[0]
        x[n - 1] = x[0]
    if nan_row is not None and n > nan_row:
        x[nan_row] = NAN
    return x


def _same(ex, want, weakest=True):
    """Extremes against the oracle's decoded lists; scores compared as values with -0.0 == +0.0 (both sides canonicalise)"""
    got = [t.tolist() if t is not None else None for t in ex]
    for k in range(6 if weakest else 4):
        assert got[k] == want[k], k
    if not weakest:
        assert got[4] is None and got[5] is None


# ---- the CPU path against the oracle
@pytest.mark.parametrize("n", [1, 2, 5, 64, 130])
def test_cpu_class_extremes_equal_the_oracle(n):
    x = int_rows(n, 8, n, nan_row=2 if n >= 64 else None)
    S = x @ x.t()
    y = int_rows(max(n - 1, 1) + 3, 8, 100 + n, nan_row=4 if n >= 64 else None)
    Sy = x @ y.t()
    cy = OO.class_patterns(y.shape[0], 50 + n)
    for name, cls in OO.class_patterns(n, n).items():
        want = OO.decoded(OO.extremes(S, cls.tolist()))
        ex = match.class_extremes(x, cls, normalize=False)
        assert ex.pos_score.dtype == torch.float32 and ex.pos_index.dtype == torch.int64 and ex.weak_index.dtype == torch.int64
        _same(ex, want)
        _same(match.class_extremes(x, cls, normalize=False, weakest=False), want, weakest=False)
        # the torch form of the oracle: the same keys
        assert [OO.as_unsigned(k) for k in OO.extremes_torch(S, cls)] == OO.extremes(S, cls.tolist()), name
        # two-set: the rows of x against the gallery y
        want2 = OO.decoded(OO.extremes(Sy, cls.tolist(), cy[name].tolist(), n_nodes=n))
        _same(match.class_extremes(x, cls, emb_b=y, classes_b=cy[name], normalize=False), want2)
    if n >= 5:
        # premises: the duplicated rows tie (the best mate of a one-class set is decided by the index) and the NaN row has nothing
        one = match.class_extremes(x, torch.zeros(n, dtype=torch.int64), normalize=False)
        assert S[0, 3] == S[0, n - 1] == S[0, 0] and one.neg_index.tolist() == [-1] * n and one.neg_score.tolist() == [-INF] * n
        if n >= 64:
            assert one.pos_index[2] == -1 and one.pos_score[2] == -INF and one.weak_score[2] == INF and 2 not in one.pos_index.tolist()


def test_cpu_rules_by_hand():
    # scores of item 0 against 1..5: mates 1, 2 (class 7) at 4 and 4 -> tie, index 1; impostors 3 (class 8) at -0.0-like 0, 4 (distractor)
    # at 0, 5 (distractor, same negative value as 4) — distractors are impostors to each other too
    x = torch.tensor([[2., 0, 0], [2., 1, 0], [2., -1, 0], [0., 0, 3], [0., 5, 0], [0., 5, 0]])
    cls = torch.tensor([7, 7, 7, 8, -2, -2])
    ex = match.class_extremes(x, cls, normalize=False)
    assert ex.pos_index.tolist() == [1, 0, 0, -1, -1, -1] and ex.pos_score.tolist() == [4, 4, 4, -INF, -INF, -INF]
    assert ex.weak_index.tolist() == [1, 2, 1, -1, -1, -1] and ex.weak_score.tolist() == [4, 3, 3, INF, INF, INF]
    assert ex.neg_index.tolist() == [3, 4, 3, 0, 5, 4] and ex.neg_score.tolist() == [0, 5, 0, 0, 25, 25]
    _same(ex, OO.decoded(OO.extremes(x @ x.t(), cls.tolist())))
    # key encoding and decoding of the oracle: -0.0 and +0.0 share a key, kind 1 undoes the complement, index >= 2^31 is "none"
    assert OO.key(-0.0, 5) == OO.key(0.0, 5) == (0x80000000 << 32) | (0xFFFFFFFF - 5)
    assert OO.decode(OO.key(-1.5, 9), 0) == (-1.5, 9) and OO.decode(OO.key(-1.5, 9, lowest=True), 1) == (-1.5, 9)
    assert OO.key(2.0, 1) > OO.key(2.0, 2) > OO.key(1.0, 0) > OO.key(-1.0, 0) > 0
    assert OO.key(1.0, 1, lowest=True) > OO.key(1.0, 2, lowest=True) > OO.key(2.0, 0, lowest=True)
    assert OO.decode(0, 0) == (-INF, -1) and OO.decode(0, 1) == (INF, -1) and OO.decode((5 << 32) | 0x7FFFFFFF, 0) == (-INF, -1)


def test_argument_validation():
    x = torch.randn(6, 8, generator=torch.Generator().manual_seed(0))
    c = torch.arange(6)
    for kw in (dict(classes=c[:5]), dict(classes=c.float()), dict(classes=c, emb_b=x), dict(classes=c, classes_b=c),
               dict(classes=c, chunk=0), dict(classes=c, compute_dtype=torch.float16), dict(classes=c + 2 ** 31)):
        with pytest.raises(PfrError):
            match.class_extremes(x, **kw)
    with pytest.raises(PfrError):
        match.class_extremes(x[0], c)


# ---- OpenSetStats against a brute-force loop
def _brute(ps, pi, ns, ni, k_of):
    """-> rank1, {f: (dir, threshold)}; k_of[f] = floor(f n) worked out by hand"""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    n_all = len(ps)
    mated = [x for x in range(n_all) if pi[x] >= 0]
    hit = [x for x in mated if ni[x] < 0 or ps[x] > ns[x] or (ps[x] == ns[x] and pi[x] < ni[x])]
    negs = sorted((f32(ns[x]) for x in range(n_all) if ni[x] >= 0), reverse=True)
    out = {}
    for f, k in k_of.items():
        if k >= len(negs):
            t = -INF
        else:
            t = float(torch.nextafter(torch.tensor(negs[k], dtype=torch.float32), torch.tensor(INF)))
            assert sum(1 for v in negs if v >= t) <= k                     # the definition: at most floor(f n) false alarms ...
            assert sum(1 for v in negs if v >= negs[k]) > k                 # ... and the float below would raise one more
        out[f] = (len([x for x in hit if f32(ps[x]) >= t]) / len(mated) if mated else NAN, t)
    return (len(hit) / len(mated) if mated else NAN), out


def _check(ps, pi, ns, ni, k_of):
    st = OpenSetStats(torch.tensor(ps), torch.tensor(pi), torch.tensor(ns), torch.tensor(ni))
    r1, pts = _brute(ps, pi, ns, ni, k_of)
    eq = lambda a, b: a == b or (a != a and b != b)
    assert eq(st.rank1(), r1)
    m = st.metrics(list(k_of))
    assert list(m.keys()) == ["rank1"] + [k for f in k_of for k in (f"DIR@FPIR={f}", f"TH@FPIR={f}")]
    for f, (d, t) in pts.items():
        assert eq(st.dir_at_fpir(f), d) and st.threshold_at_fpir(f) == t and eq(st.fnir_at_fpir(f), 1.0 - d), f
        assert eq(m[f"DIR@FPIR={f}"], d) and m[f"TH@FPIR={f}"] == t
        if t > -INF:
            assert st.fpir(t) <= f and st.fpir(float(torch.nextafter(torch.tensor(t), torch.tensor(-INF)))) > f
    return st


def test_open_set_stats_against_brute_force():
    # ten probes; 0..5 mated; impostor scores with a duplicate (0.5 twice) where the thresholds fall
    ps = [0.9, 0.8, 0.5, 0.5, 0.3, 0.7, -INF, -INF, -INF, -INF]
    pi = [1, 0, 3, 2, 5, 4, -1, -1, -1, -1]
    ns = [0.4, 0.85, 0.5, 0.5, 0.2, 0.6, 0.5, 0.1, 0.45, 0.3]
    ni = [6, 7, 9, 1, 0, 8, 3, 2, 1, 0]
    # hits: 0, 4, 5 (mate above), 3 (tie 0.5 / 0.5, mate index 2 < impostor index 1? no: 2 > 1 -> a miss), 2 (tie, 3 < 9 -> a hit)
    st = _check(ps, pi, ns, ni, {0.1: 1, 0.0: 0, 0.3: 3, 0.35: 3, 1.0: 10, 0.99: 9})
    assert st.hit.tolist() == [True, False, True, False, True, True] + [False] * 4 and st.rank1() == 4 / 6 and st.n == 10
    # floor(f n) = 1: above the second largest impostor score 0.6; = 3: the duplicates 0.5 at the cut — the threshold moves above ALL of them
    assert st.threshold_at_fpir(0.1) == float(torch.nextafter(torch.tensor(0.6), torch.tensor(INF)))
    assert st.threshold_at_fpir(0.3) == float(torch.nextafter(torch.tensor(0.5), torch.tensor(INF))) and st.fpir(st.threshold_at_fpir(0.3)) == 0.2
    assert st.threshold_at_fpir(0.0) == float(torch.nextafter(torch.tensor(0.85), torch.tensor(INF))) and st.threshold_at_fpir(1.0) == -INF
    assert st.dir_at_fpir(1.0) == st.rank1() and st.dir_at_fpir(0.1) == 2 / 6 and st.dir_at_fpir(0.0) == 1 / 6
    # f n taken exactly: 0.29 * 100 is 29 (the double product is 28.999…)
    big = OpenSetStats(torch.zeros(100), torch.full((100,), -1), torch.arange(100.), torch.zeros(100, dtype=torch.int64))
    assert big.threshold_at_fpir(0.29) == float(torch.nextafter(torch.tensor(70.0), torch.tensor(INF))) and big.fpir(big.threshold_at_fpir(0.29)) == 0.29
    # no mated probe: NaN rates, thresholds still defined
    st0 = _check([-INF] * 3, [-1] * 3, [0.1, 0.2, 0.3], [1, 2, 0], {0.5: 1, 0.1: 0})
    assert math.isnan(st0.rank1()) and math.isnan(st0.dir_at_fpir(0.5)) and st0.n_mated == 0
    # no impostor at all (one class): every mated probe is a hit, n = 0, the threshold is -inf
    st1 = _check([0.5, 0.6], [1, 0], [-INF, -INF], [-1, -1], {0.01: 0, 0.5: 0})
    assert st1.rank1() == 1.0 and st1.n == 0 and st1.threshold_at_fpir(0.01) == -INF and st1.dir_at_fpir(0.01) == 1.0 and math.isnan(st1.fpir(0.0))
    with pytest.raises(ValueError):
        OpenSetStats(torch.zeros(3), torch.zeros(3), torch.zeros(2), torch.zeros(3))


def test_label_suspects_order():
    E = match.Extremes
    ps = torch.tensor([0.9, 0.2, 0.5, 0.5, -INF, 0.1, 0.4, 0.3])
    pi = torch.tensor([1, 0, 3, 2, -1, 6, 5, 9])
    ns = torch.tensor([0.3, 0.6, 0.5, 0.5, 0.99, 0.5, 0.8, -INF])
    ni = torch.tensor([5, 6, 1, 7, 0, 0, 1, -1])
    # 1: 0.6 > 0.2 (gap 0.4); 2: tie, impostor index 1 < mate index 3 (gap 0); 3: tie, impostor 7 > mate 2 (no); 4: no mate (no);
    # 5: gap 0.4 (float32: 0.5 - 0.1 = 0.4 exactly the same float as 0.6 - 0.2? compared as computed); 6: gap 0.4; 7: no impostor (no)
    got = match.label_suspects(E(ps, pi, ns, ni, None, None))
    assert got.dtype == torch.int64 and sorted(got.tolist()) == [1, 2, 5, 6] and got.tolist()[-1] == 2
    gap = (ns - ps)
    want = sorted([1, 2, 5, 6], key=lambda x: (-float(gap[x]), x))
    assert got.tolist() == want
    assert match.label_suspects(E(ps[:1], pi[:1], ns[:1], ni[:1], None, None)).tolist() == []
    # end to end on rows: item 2 carries the wrong label (it lies with the class of 3 and 4), and drags 3 and 4 along
    x = torch.tensor([[4., 0], [4., 1], [0., 4], [1., 4], [4., -1]])
    ex = match.class_extremes(x, torch.tensor([0, 0, 0, 1, 1]), normalize=False)
    assert match.label_suspects(ex).tolist() == [3, 4, 2]          # gaps 16 - 0, 16 - 0 (the index decides), 16 - 4
    assert (ex.neg_score - ex.pos_score)[[3, 4, 2]].tolist() == [16.0, 16.0, 12.0]
    m = match.open_set_metrics(x, torch.tensor([0, 0, 0, 1, 1]), fpir=(0.5,), normalize=False)
    assert m == OpenSetStats(ex.pos_score, ex.pos_index, ex.neg_score, ex.neg_index).metrics((0.5,)) and m["rank1"] == 2 / 5


# ---- Controller and eval_fe.py
def open_set_keys(fpirs):
    return (["OpenSet rank1"] + [f"OpenSet DIR@FPIR={f}" for f in fpirs] + [f"OpenSet TH@FPIR={f}" for f in fpirs] + ["OpenSet suspects"])


@pytest.mark.parametrize("method", ["_evaluate", "test_epoch_end"])
def test_controller_open_set_keys_and_values(method):
    from test_cluster_host import _controller, separated_set
    emb, classes = separated_set()
    base_c, batches, _, _ = _controller({"dbscan": dict(thresholds=[0.9], min_samples=3)}, emb, classes)
    base = getattr(base_c, method)([batches])["Val"]
    assert not any(k.startswith("OpenSet") for k in base)                              # opt-in
    fpirs = [0.1, 0.01]
    c, batches, _, _ = _controller({"dbscan": dict(thresholds=[0.9], min_samples=3), "open_set": dict(fpir=fpirs)}, emb, classes)
    m = getattr(c, method)([batches])["Val"]
    assert list(m.keys()) == list(base.keys()) + open_set_keys(fpirs)                  # appended after the DBSCAN keys
    for k, v in base.items():
        assert m[k] == v or (v != v and m[k] != m[k]), k
    ex = match.class_extremes(emb, classes, weakest=False)
    st = OpenSetStats(ex.pos_score, ex.pos_index, ex.neg_score, ex.neg_index)
    assert m["OpenSet rank1"] == st.rank1() == 1.0 and m["OpenSet suspects"] == 0      # tight, well separated classes of 3
    for f in fpirs:
        assert m[f"OpenSet DIR@FPIR={f}"] == st.dir_at_fpir(f) == 1.0
        assert m[f"OpenSet TH@FPIR={f}"] == (st.threshold_at_fpir(f) + 1.0) / 2.0 and 0.0 < m[f"OpenSet TH@FPIR={f}"] < 0.9
    # the default rates, and a wrong label shows up as suspects
    bad = classes.clone()
    bad[0] = 5
    c2, batches2, _, _ = _controller({"open_set": dict()}, emb, bad)
    m2 = getattr(c2, method)([batches2])["Val"]
    assert list(m2.keys())[-6:] == open_set_keys([0.1, 0.01]) and m2["OpenSet suspects"] >= 1 and m2["OpenSet rank1"] < 1.0


def test_eval_fe_flag_reaches_the_config(monkeypatch):
    sys.path.insert(0, ROOT)
    import eval_fe
    seen = {}

    class FakeController:
        def __init__(self, config):
            seen["open_set"] = config.get("open_set")

    class FakeTrainer:
        def test(self, controller):
            return "tested"

    monkeypatch.setattr(eval_fe, "Controller", FakeController)
    monkeypatch.setattr(eval_fe, "configure_trainer", lambda *a, **k: FakeTrainer())
    with tempfile.TemporaryDirectory() as td:
        cfg = os.path.join(td, "cfg.py")
        open(cfg, "w").write("n_epochs = 1\ndevice = 'cpu'\n")
        assert eval_fe.main(["-c", cfg, "--open-set", "0.1", "0.01"]) == "tested"
        assert seen["open_set"] == dict(fpir=[0.1, 0.01])
        assert eval_fe.main(["-c", cfg]) == "tested"
        assert seen["open_set"] is None
        with pytest.raises(SystemExit):
            eval_fe.main(["-c", cfg, "--open-set", "high"])
        with pytest.raises(SystemExit):
            eval_fe.main(["-c", cfg, "--open-set"])


def test_open_set_config_imports_and_sets_the_key():
    from pets_face_recognition_amd.utils import get_config
    cfg = get_config(os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic", "fe_r18_mi355x_openset.py"))
    assert cfg.get("open_set") == dict(fpir=[0.1, 0.01]) and cfg.get("dbscan") is None


# ---- C-ABI
def test_header_declares_the_entry_points():
    from pets_face_recognition_amd._hip.lib import LIB_PATH, parse_header
    protos = parse_header()
    assert {"pfr_class_extremes", "pfr_extremes_decode"} <= set(protos)
    assert protos["pfr_class_extremes"][2] == ["a", "a_scale", "Na", "a_off", "b", "b_scale", "Nb", "b_off", "dtype", "D", "cls_a", "cls_b",
                                               "both_sides", "best_pos", "best_neg", "worst_pos", "n_nodes", "stream"]
    assert protos["pfr_extremes_decode"][2] == ["keys", "n", "kind", "score", "index", "stream"]
    inc = open(os.path.join(os.path.dirname(LIB_PATH), "pfr_thunks_gen.inc")).read()
    for name in ("pfr_class_extremes", "pfr_extremes_decode"):
        assert f'{{"{name}", th_{name}}}' in inc
    hdr = open(os.path.join(ROOT, "include", "pfr_hip.h")).read()
    assert "cls_a[i] == cls_b[j] and" in hdr and "(~ord(s) << 32) | (0xffffffff - partner)" in hdr and "leave-one-out" in hdr
    # the shared key header: one definition of the order-preserving map
    csrc = os.path.dirname(LIB_PATH)
    assert "db_score_key" in open(os.path.join(csrc, "pfr_scorekey.h")).read()
    for src in ("pfr_dbscan.hip", "pfr_extremes.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "pfr_scorekey.h"' in text and "unsigned int db_score_key(float" not in text


def test_argument_checks_fail_before_any_launch():
    from pets_face_recognition_amd._hip import lib
    # pointers are never dereferenced on the host: every call fails a check first (16 is a non-null address that is not device memory)
    def ext(a=16, Na=8, a_off=0, b=0, Nb=0, b_off=0, dtype=1, D=64, cls_a=16, cls_b=16, both=0, pos=16, neg=16, worst=16, n_nodes=64, sa=0, sb=0):
        return lib.pfr_class_extremes(a, sa, Na, a_off, b, sb, Nb, b_off, dtype, D, cls_a, cls_b, both, pos, neg, worst, n_nodes, 0)
    bad = [dict(dtype=3), dict(dtype=-1), dict(D=48), dict(D=0), dict(dtype=0, D=48), dict(dtype=2, D=64),                   # dtype / D
           dict(Na=-1), dict(b=16, Nb=-1), dict(n_nodes=-1), dict(a_off=-1), dict(b=16, Nb=8, b_off=-1),                        # negative sizes
           dict(n_nodes=7), dict(a_off=57), dict(b=16, Nb=8, b_off=57, both=1),                                                # off + rows > n_nodes
           dict(a_off=2 ** 31 - 8, n_nodes=2 ** 31 - 1), dict(b=16, Nb=8, b_off=2 ** 31 - 8, n_nodes=2 ** 31 - 1, both=1),
           dict(b=16, Nb=8, b_off=2 ** 31 - 8),                                                                                # the partner passes 2^31 - 1
           dict(a=0), dict(cls_a=0), dict(b=16, Nb=8, cls_b=0), dict(pos=0), dict(neg=0),                                       # null pointers
           dict(dtype=2, D=128), dict(dtype=2, D=128, sa=16, b=16, Nb=8),                                                      # int8 without scales
           dict(), dict(worst=0), dict(b=16, Nb=8), dict(b=16, Nb=8, b_off=56, both=1)]                                        # host pointers
    for kw in bad:
        with pytest.raises(PfrError):
            ext(**kw)
    # one-sided two-set form: b_off + Nb may pass n_nodes (the b side has no output) — it fails later, on the pointers, not on the geometry
    with pytest.raises(PfrError, match="device memory"):
        ext(b=16, Nb=8, b_off=1000)
    with pytest.raises(PfrError, match="n_nodes"):
        ext(b=16, Nb=8, b_off=1000, both=1)
    # nothing to do: no pointer is looked at
    assert ext(Na=0, a=0, cls_a=0) == 0 and ext(Na=1, pos=0) == 0 and ext(b=16, Nb=0, neg=0) == 0

    def dec(keys=16, n=8, kind=0, score=16, index=16):
        return lib.pfr_extremes_decode(keys, n, kind, score, index, 0)
    for kw in (dict(n=-1), dict(kind=2), dict(kind=-1), dict(keys=0), dict(score=0), dict(index=0), dict()):
        with pytest.raises(PfrError):
            dec(**kw)
    assert dec(n=0, keys=0, score=0, index=0) == 0
