"""The CPU oracle (oracle/) against the golden vectors generated from the reference's own modules
(oracle/make_golden.py) — and the product's CPU (torch) execution path against the same vectors."""
import math
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _arc_cases():
    G = np.load(os.path.join(GOLD, "arcface.npz"))
    for name, arc, easy in [("arc_hard", True, False), ("arc_easy", True, True), ("cosface", False, False),
                            ("arc_hard_400", True, False)]:
        for gamma in (0, 2):
            key = f"{name}_g{gamma}"
            if key + "_x" in G:
                yield G, key, arc, easy, gamma


def _logits_close(lo, G, key, arc, easy, rtol=1e-6, atol=1e-5):
    """torch.allclose(lo, golden, rtol, atol), with the bound of each label entry scaled by how much the margin function amplifies
    a change of the cosine there (|d shifted / d cos|, never below 1).  Near cos = 1 ArcFace's cos(θ + m) has slope
    cos m + sin m · cos θ / sin θ (≈ 56 at cos θ = 0.99996), so the one-ulp spread of the cosine GEMM between BLAS code paths
    (summation order; e.g. MKL on non-Intel hosts) becomes tens of ulps of that logit.  Every other entry keeps the plain bound."""
    gold = torch.tensor(G[key + "_logits"])
    tol = atol + rtol * gold.abs()
    if arc:
        m = float(G[key + "_m"])
        x, w = torch.tensor(G[key + "_x"]).double(), torch.tensor(G[key + "_w"]).double()
        rows = torch.arange(x.shape[0])
        c = (torch.nn.functional.normalize(x, dim=1) @ torch.nn.functional.normalize(w, dim=1).t())[rows, torch.tensor(G[key + "_label"]).long()]
        on_margin = c > 0 if easy else c > math.cos(math.pi - m)
        slope = math.cos(m) + math.sin(m) * c / (1.0 - c * c).clamp_min(1e-30).sqrt()
        scale = torch.where(on_margin, slope.abs(), torch.ones_like(c)).clamp_min(1.0).float()
        tol[rows, torch.tensor(G[key + "_label"]).long()] *= scale
    return bool(((lo.detach() - gold).abs() <= tol).all())


def test_oracle_arcface_matches_reference_vectors():
    from oracle import arcface_ref
    n = 0
    for G, key, arc, easy, gamma in _arc_cases():
        x = torch.tensor(G[key + "_x"]).requires_grad_(True)
        w = torch.tensor(G[key + "_w"]).requires_grad_(True)
        y = torch.tensor(G[key + "_label"])
        s, m = float(G[key + "_s"]), float(G[key + "_m"])
        lo = arcface_ref.arc_margin_logits(x, w, y, s, m, easy) if arc else arcface_ref.add_margin_logits(x, w, y, s, m)
        loss = arcface_ref.focal_loss(lo, y, gamma)
        loss.backward()
        assert _logits_close(lo, G, key, arc, easy), key
        assert abs(loss.item() - float(G[key + "_loss"])) < 1e-5
        assert torch.allclose(x.grad, torch.tensor(G[key + "_dx"]), rtol=1e-4, atol=1e-6)
        assert torch.allclose(w.grad, torch.tensor(G[key + "_dw"]), rtol=1e-4, atol=1e-6)
        n += 1
    assert n == 7


def test_product_cpu_path_losses_match_reference_vectors():
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    for G, key, arc, easy, gamma in _arc_cases():
        C = G[key + "_w"].shape[0]
        wrap = SoftmaxBasedMetricLearning(torch.nn.Identity(), C, 512, is_focal=True, loss_kwargs=dict(gamma=gamma),
                                          arc_margin=arc, easy_margin=easy)
        with torch.no_grad():
            wrap.add_margin.weight.copy_(torch.tensor(G[key + "_w"]))
        x = torch.tensor(G[key + "_x"]).requires_grad_(True)
        r = wrap(x, torch.tensor(G[key + "_label"]))
        r["loss"].backward()
        assert _logits_close(r["logits"], G, key, arc, easy), key
        assert abs(r["loss"].item() - float(G[key + "_loss"])) < 1e-5
        assert torch.allclose(x.grad, torch.tensor(G[key + "_dx"]), rtol=1e-4, atol=1e-6)
        assert set(r.keys()) == {"loss", "emb", "logits"}
    # label=None returns the bare embedding; list input is embedded item by item
    assert torch.equal(wrap(x.detach()), x.detach())
    assert wrap([x.detach()[:3], x.detach()[3:5]]).shape[0] == 5


def _alpha_case(G, name, device):
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    C = G[name + "_w"].shape[0]
    wrap = SoftmaxBasedMetricLearning(torch.nn.Identity(), C, 512, is_focal=True, loss_kwargs=dict(gamma=float(G[name + "_gamma"]), alpha=True),
                                      arc_margin=name.startswith("arc"))
    assert wrap.focal_loss.adaptive_flag and wrap._fusable(torch.zeros(1, device=device)) is None
    if device != "cpu":
        wrap.add_margin.compute_dtype = torch.float32
    wrap = wrap.to(device)
    with torch.no_grad():
        wrap.add_margin.weight.copy_(torch.tensor(G[name + "_w"]))
        wrap.focal_loss.alpha.copy_(torch.tensor(G[name + "_alpha"]))
    x = torch.tensor(G[name + "_x"]).to(device).requires_grad_(True)
    r = wrap(x, torch.tensor(G[name + "_label"]).to(device))
    r["loss"].backward()
    return wrap, x, r


def test_product_cpu_path_adaptive_alpha_focal_matches_reference_vectors():
    """FocalLoss(alpha=True) (reference losses/losses.py:13-24: learnable per-class logit scale; no FE config uses it) through the product's
    SoftmaxBasedMetricLearning on CPU tensors against vectors produced by the reference class itself (oracle/make_golden.py:gen_arcface_alpha)."""
    G = np.load(os.path.join(GOLD, "arcface_alpha.npz"))
    for name in ("arc_hard_alpha", "cosface_alpha"):
        wrap, x, r = _alpha_case(G, name, "cpu")
        assert torch.allclose(r["logits"], torch.tensor(G[name + "_logits"]), rtol=1e-6, atol=1e-5), name
        assert abs(r["loss"].item() - float(G[name + "_loss"])) < 1e-5
        assert torch.allclose(x.grad, torch.tensor(G[name + "_dx"]), rtol=1e-4, atol=1e-6)
        assert torch.allclose(wrap.add_margin.weight.grad, torch.tensor(G[name + "_dw"]), rtol=1e-4, atol=1e-6)
        assert torch.allclose(wrap.focal_loss.alpha.grad, torch.tensor(G[name + "_dalpha"]), rtol=1e-4, atol=1e-6)


def test_oracle_recall_matches_reference_controller():
    from oracle import match_ref
    G = np.load(os.path.join(GOLD, "recall.npz"))
    for name in ("n256", "n400"):
        emb, cls = torch.tensor(G[f"{name}_emb"]), torch.tensor(G[f"{name}_classes"])
        loop = match_ref.recall_at_k_loop(emb[:128], cls[:128], (10, 100))      # literal loop on a prefix (speed)
        mat = match_ref.recall_at_k_matrix(emb[:128], cls[:128], (10, 100))
        assert loop == mat
        full = match_ref.recall_at_k_matrix(emb, cls, (10, 100))
        for k in (10, 100):
            assert full[k] == G[f"{name}_recall{k}_counts"].tolist()
            assert abs(full[k][0] / full[k][1] - float(G[f"{name}_recall{k}_ref"])) < 1e-12
    # product CPU path
    from pets_face_recognition_amd.match import recall_at_k, pair_similarity
    emb, cls = torch.tensor(G["n256_emb"]), torch.tensor(G["n256_classes"])
    got = recall_at_k(emb, cls, (10, 100))
    assert [got[10], got[100]] == [G["n256_recall10_counts"].tolist(), G["n256_recall100_counts"].tolist()]
    pairs = G["n256_pairs"]
    assert torch.allclose(pair_similarity(emb, pairs[:, 0], pairs[:, 1]), torch.tensor(G["n256_pair_scores"]), atol=1e-6)


def test_swin_restatement_matches_reference_vectors():
    import pets_face_recognition_amd.models as M
    G = np.load(os.path.join(GOLD, "swin_t.npz"))
    torch.manual_seed(int(G["seed"]))
    m = M.swin_t(num_classes=512)
    assert sum(p.numel() for p in m.parameters()) == int(G["n_params"])
    assert sorted(m.state_dict().keys()) == list(G["keys"])
    x = torch.rand(2, 3, 224, 224, generator=torch.Generator().manual_seed(int(G["x_seed"])))
    with torch.no_grad():
        y = m(x)
        s1 = m.stage1(x)
    assert torch.allclose(y, torch.tensor(G["emb"]), rtol=1e-4, atol=1e-5)
    assert torch.allclose(s1[:, :8, :6, :6], torch.tensor(G["stage1_sample"]), rtol=1e-4, atol=1e-5)


def test_resnet_restatement_self_checks():
    """torchvision is absent: the ResNet oracle is 'parity unpinned' at that boundary; self-checks per SURVEY §8c"""
    from oracle import resnet_ref
    import pets_face_recognition_amd.models as M
    for arch, nparam, nkeys in (("resnet50", 24557120, 320), ("resnet18", 11439168, 122)):
        sd = resnet_ref.init_state_dict(arch, 512, seed=0)
        assert len(sd) == nkeys
        assert sum(v.numel() for k, v in sd.items() if k in resnet_ref.param_names(sd)) == nparam
        m = getattr(M, arch)()
        m.fc = torch.nn.Linear(m.fc.in_features, 512)
        assert list(m.state_dict().keys()) == list(sd.keys())          # torchvision key names and order
        m.load_state_dict(sd)
    # product CPU path (plain torch.nn layers) == functional oracle
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    m.train()
    new = {}
    ref = resnet_ref.forward(sd, x, "resnet18", train=True, new_stats=new)
    got = m(x)
    assert torch.allclose(got, ref, rtol=1e-4, atol=1e-5)
    assert torch.allclose(m.bn1.running_mean, new["bn1.running_mean"], atol=1e-6)


def _hf_resnet(arch, sd):
    """The same weights loaded into Hugging Face transformers' ResNetModel — an independent third-party implementation of
    the published ResNet v1.5 architecture (the one torchvision.models.resnet* implements; stride on the 3x3 conv)."""
    from transformers import ResNetConfig, ResNetModel
    if arch == "resnet50":
        cfg = ResNetConfig(num_channels=3, embedding_size=64, hidden_sizes=[256, 512, 1024, 2048], depths=[3, 4, 6, 3],
                           layer_type="bottleneck", hidden_act="relu", downsample_in_first_stage=False,
                           downsample_in_bottleneck=False)
        nconv = 3
    else:
        cfg = ResNetConfig(num_channels=3, embedding_size=64, hidden_sizes=[64, 128, 256, 512], depths=[2, 2, 2, 2],
                           layer_type="basic", hidden_act="relu", downsample_in_first_stage=False)
        nconv = 2
    hf = ResNetModel(cfg)
    new = {}

    def put(dst, src_conv, src_bn):
        new[dst + ".convolution.weight"] = sd[src_conv + ".weight"]
        for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
            new[dst + ".normalization." + k] = sd[src_bn + "." + k]

    put("embedder.embedder", "conv1", "bn1")
    for L, depth in enumerate(cfg.depths):
        for b in range(depth):
            tv, h = f"layer{L + 1}.{b}", f"encoder.stages.{L}.layers.{b}"
            for i in range(nconv):
                put(f"{h}.layer.{i}", f"{tv}.conv{i + 1}", f"{tv}.bn{i + 1}")
            if f"{tv}.downsample.0.weight" in sd:
                put(f"{h}.shortcut", f"{tv}.downsample.0", f"{tv}.downsample.1")
    missing, unexpected = hf.load_state_dict(new, strict=True), None
    return hf


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_resnet_restatement_matches_hf_transformers_resnet(arch):
    """torchvision is not installable here, so the restated backbone is additionally cross-checked against the ResNet of
    Hugging Face transformers (installed in this image): same seeded weights → same pooled features → same embedding,
    in eval mode and in train mode (batch statistics + running-statistics update)."""
    pytest.importorskip("transformers")
    from oracle import resnet_ref
    import pets_face_recognition_amd.models as M
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = resnet_ref.init_state_dict(arch, 512, seed=4)
    g = torch.Generator().manual_seed(9)
    for k in list(sd):                       # non-trivial running statistics for the eval-mode comparison
        if k.endswith("running_mean"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.1
        elif k.endswith("running_var"):
            sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
    x = torch.rand(3, 3, 96, 96, generator=g)
    hf = _hf_resnet(arch, sd)
    prod = getattr(M, arch)()
    prod.fc = torch.nn.Linear(prod.fc.in_features, 512)
    prod.load_state_dict(sd)
    for train in (False, True):
        hf.train(train)
        prod.train(train)
        new = {}
        with torch.no_grad():
            pooled = hf(x).pooler_output.flatten(1)
            emb_hf = pooled @ sd["fc.weight"].t() + sd["fc.bias"]
            emb_or = resnet_ref.forward(sd, x, arch, train=train, new_stats=new)
            emb_pr = prod(x)
        assert torch.allclose(emb_or, emb_hf, rtol=2e-4, atol=2e-5), (arch, train, (emb_or - emb_hf).abs().max())
        assert torch.allclose(emb_pr, emb_hf, rtol=2e-4, atol=2e-5), (arch, train)
        if train:
            h = hf.state_dict()
            assert torch.allclose(new["bn1.running_mean"], h["embedder.embedder.normalization.running_mean"], atol=1e-6)
            last = f"layer4.{1 if arch == 'resnet18' else 2}.bn{2 if arch == 'resnet18' else 3}.running_var"
            hl = f"encoder.stages.3.layers.{1 if arch == 'resnet18' else 2}.layer.{1 if arch == 'resnet18' else 2}.normalization.running_var"
            assert torch.allclose(new[last], h[hl], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_resnet_restatement_matches_hf_fixture(arch):
    """tests/golden/resnet_hf.npz (oracle/make_golden.py resnet_hf): embeddings an INDEPENDENT ResNet v1.5 implementation
    (Hugging Face transformers) produced for seeded weights; the oracle and the product's CPU path regenerate the weights
    from the seed and must reproduce them — no transformers import needed here."""
    from oracle import resnet_ref
    from oracle.make_golden import resnet_hf_inputs
    import pets_face_recognition_amd.models as M
    G = np.load(os.path.join(GOLD, "resnet_hf.npz"))
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd, x = resnet_hf_inputs(arch)
    prod = getattr(M, arch)()
    prod.fc = torch.nn.Linear(prod.fc.in_features, 512)
    prod.load_state_dict(sd)
    for mode in ("eval", "train"):
        want = torch.tensor(G[f"{arch}_{mode}_emb"])
        new = {}
        with torch.no_grad():
            got_o = resnet_ref.forward(sd, x, arch, train=(mode == "train"), new_stats=new)
            got_p = prod.train(mode == "train")(x)
        assert torch.allclose(got_o, want, rtol=2e-4, atol=2e-5), (arch, mode)
        assert torch.allclose(got_p, want, rtol=2e-4, atol=2e-5), (arch, mode)
    assert torch.allclose(new["bn1.running_mean"], torch.tensor(G[f"{arch}_bn1_running_mean_after"]), atol=1e-6)


@pytest.mark.parametrize("name", ["n256", "n400", "ties"])
def test_roc_auc_and_accuracy_equal_reference_controller(name):
    """'ROC AUC' and 'Accuracy' printed by the reference's Controller.test_epoch_end (controller.py:67-75, 206-211) on the
    fixture's pairs vs engine/metrics.py (a12 / a14), through Controller.compute_accuracy's own signature too."""
    from pets_face_recognition_amd.engine import metrics as M
    from pets_face_recognition_amd.engine.controller import Controller
    G = np.load(os.path.join(GOLD, "recall.npz"))
    scores = torch.tensor(G[f"{name}_pair_scores"])
    labels = torch.tensor(G[f"{name}_plabels"])
    fpr, tpr, thr = M.roc_curve(scores, labels)
    assert abs(M.auroc(scores, labels) - float(G[f"{name}_auc_ref"])) < 1e-6   # the reference prints a float32 tensor
    acc = Controller.compute_accuracy(scores, labels, thr, fpr, 1 - tpr)
    assert abs(acc - float(G[f"{name}_acc_ref"])) < 1e-9


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_pair_generator_seeded_equivalent_to_reference(name):
    """PairGenerator(dataset, gen_number, gen_ratio, None, seed, users): same pairs, labels, correction table and
    corrected_indices as the reference's class produced for the same arguments (tests/golden/pairs.npz)."""
    from pets_face_recognition_amd.data_loading import PairGenerator
    G = np.load(os.path.join(GOLD, "pairs.npz"))
    counts, perm = G[f"{name}_counts"], G[f"{name}_perm"]
    u2i, o = {}, 0
    for u, c in enumerate(counts):
        u2i[u] = sorted(int(v) for v in perm[o:o + c])
        o += int(c)

    class DS:
        uid_to_indices = u2i

        def __len__(self):
            return int(counts.sum())

    gen_number, seed = (int(v) for v in G[f"{name}_args"])
    pg = PairGenerator(DS(), None if gen_number < 0 else gen_number, float(G[f"{name}_ratio"]), None, seed,
                       [int(u) for u in G[f"{name}_users"]])
    assert np.array_equal(np.array(pg.pairs), G[f"{name}_pairs"])
    assert np.array_equal(np.asarray(pg.labels), G[f"{name}_labels"])
    assert sorted(pg.correction) == G[f"{name}_corr_keys"].tolist()
    assert [pg.correction[k] for k in sorted(pg.correction)] == G[f"{name}_corr_vals"].tolist()
    assert np.array_equal(np.array(pg.corrected_indices), G[f"{name}_corrected"])
    assert pg.indices == [tuple(r[:2]) for r in G[f"{name}_pairs"].tolist()]


def _calc_scores_fixture():
    z = np.load(os.path.join(GOLD, "calc_scores.npz"))
    q = tuple(z[k] for k in ("q_head", "q_head_seg", "q_body", "q_body_seg", "q_type"))
    g = tuple(z[k] for k in ("g_head", "g_head_seg", "g_body", "g_body_seg", "g_type"))
    return z, q, g


def test_calc_scores_restatement_equals_reference_rows():
    """oracle/match_ref.calc_scores_reference vs the rows generate_tsv.py's own calc_scores produced (fusion rule, type
    filter, skipped pairs, stable descending order, top-100 answers, top-1 / mean-3 / mean-10 columns)"""
    from oracle.match_ref import calc_scores_reference
    z, q, g = _calc_scores_fixture()
    rows = calc_scores_reference(q, g)
    assert [r[0] for r in rows] == z["rows_query"].tolist()
    assert len(rows) < len(q[4])                     # the fixture holds query cards without any usable modality
    for r, t1, m3, m10, ans in zip(rows, z["top1"], z["mean3"], z["mean10"], z["answer"]):
        assert abs(r[1] - t1) < 1e-6 and abs(r[2] - m3) < 1e-6 and abs(r[3] - m10) < 1e-6
        assert r[4] == ans[ans >= 0].tolist()
    # the fixture exercises every branch of the rule
    assert any((a >= 0).sum() < 100 for a in z["answer"]) and any((a >= 0).sum() == 100 for a in z["answer"])


def _evaluate_case(name, device="cpu", match_dtype=torch.float32, similarity_f=None):
    """run the product Controller._evaluate on one set of tests/golden/evaluate.npz → (metrics dict, confusion matrix, golden)"""
    import tempfile
    from pets_face_recognition_amd.engine.controller import Controller
    E = np.load(os.path.join(GOLD, "evaluate.npz"))
    src = E if name == "edge" else np.load(os.path.join(GOLD, "recall.npz"))
    emb = torch.tensor(src[f"{name}_emb"])
    classes = torch.tensor(src[f"{name}_classes"])
    pairs = [tuple(p) for p in src[f"{name}_pairs"].tolist()]
    plabels = src[f"{name}_plabels"].tolist()

    class PG:
        corrected_indices = pairs
        labels = plabels

    def default_sim(ps):
        t1 = torch.stack([p[0] for p in ps]); t2 = torch.stack([p[1] for p in ps])
        return (torch.nn.functional.cosine_similarity(t1, t2) + 1) / 2
    default_sim._is_default_cosine = True

    class Cfg(dict):
        def pair_generator(self, i):
            return "Val", PG

    N = emb.shape[0]
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(1))
    batches = [{"emb": emb[perm][i:i + 20].to(device), "label": classes[perm][i:i + 20].to(device), "index": perm[i:i + 20].to(device)}
               for i in range(0, N, 20)]
    with tempfile.TemporaryDirectory() as td:
        cfg = Cfg(thrs=E["thrs"], k=E["k"].tolist(), far_thr=E["far_thr"].tolist(), frr_thr=E["frr_thr"].tolist(), img_dir=td)
        cfg.similarity_f = similarity_f or default_sim
        cfg.match_dtype = match_dtype
        c = Controller.__new__(Controller)
        torch.nn.Module.__init__(c)
        c.logger, c.current_epoch, c.last_metrics, c.config = None, 0, {}, cfg
        m = c._evaluate([batches])["Val"]
    gold = dict(zip(E[f"{name}_keys"].tolist(), E[f"{name}_values"].tolist()))
    return m, c.last_confmat["Val"], gold, E[f"{name}_confmat"].tolist()


def check_evaluate_against_reference(m, cm, gold, gold_cm, name):
    """key for key (same keys, same order — incl. the TAR@FAR / TRR@FRR keys the reference SKIPS when the threshold is 0 or 1);
    ratios of Python ints to 1e-12, the values the reference prints from float32 tensors to 1e-6.  Recall@K under exact score ties is
    undefined in the reference (unstable argsort, controller.py:155): the "ties" set still reproduces the golden for every K, the
    "edge" set (ties across identities at the cut) is checked against the oracle's documented tie rule."""
    assert list(m.keys()) == list(gold.keys()), (list(m.keys()), list(gold.keys()))
    for k, v in gold.items():
        if name == "edge" and k.startswith("Recall@K="):
            # four identical rows of four identities: which of them the reference's unstable argsort ranks first is arbitrary;
            # the product's documented rule (lower index first) is pinned by the oracle instead
            from oracle import match_ref
            E = np.load(os.path.join(GOLD, "evaluate.npz"))
            kk = int(k.split("=")[1])
            x, y = match_ref.recall_at_k_matrix(torch.tensor(E["edge_emb"]), torch.tensor(E["edge_classes"]), (kk,))[kk]
            assert m[k] == x / y, (name, k, m[k], x / y)
            continue
        f32 = k in ("ROC AUC", "AveragePrecision", "Opt thr") or k.startswith("TH@") or " thr=" in k   # float32 tensors' .item()
        tol = 1e-6 if f32 else 1e-12
        assert abs(m[k] - v) <= tol, (name, k, m[k], v)
    assert cm == gold_cm, (name, cm, gold_cm)


@pytest.mark.parametrize("name", ["n256", "n400", "ties", "edge"])
def test_evaluate_metrics_dict_equals_reference_evaluate(name):
    """Controller._evaluate (CPU tensors) vs the metrics the REFERENCE's own Controller._evaluate printed for the same embeddings,
    pairs, thrs / k / far_thr / frr_thr (engine/controller.py:95-183 run by oracle/make_golden.py gen_evaluate)."""
    check_evaluate_against_reference(*_evaluate_case(name), name)
