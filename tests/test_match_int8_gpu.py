"""int8 selection of the gallery match (match.cosine_topk(compute_dtype=torch.int8)): the quantiser and the selection scores against a host
restatement of their definitions (include/pfr_hip.h at pfr_quantize_rows_i8), bit for bit; the fused / unfused / overflow schedules; the
certified default path against the f32 path; the prepared handle; candR@K against the reference's counts; the 1 M config-5 gallery."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
I8 = torch.int8


def _quantize_host(xf):
    """the quantiser's definition on fp32 rows x̂ (host): m = max|x̂|, r = 127 / m, q = rint(x̂ r) (half to even), s = m / 127;
    r = +inf -> zero row, s = 0"""
    xf = xf.cpu()
    m = xf.abs().amax(dim=1)
    r = torch.tensor(127.0, dtype=torch.float32) / m
    live = torch.isfinite(r)
    rq = torch.where(live, r, torch.zeros_like(r))
    q = torch.round(xf * rq[:, None]).to(torch.int8)
    s = torch.where(live, m / torch.tensor(127.0, dtype=torch.float32), torch.zeros_like(m))
    return q, s


def _selection_host(q8, qs, g8, gs, k, exclude_self=False):
    """top-k by the selection score ((float) acc * s_q) * s_g, acc = Σ q_i g_i; sorted by (score desc, index asc).  acc is formed in
    float64: every product and partial sum is an integer below 2^53, so the matmul is exact in any summation order (= the int64 product)."""
    acc = (q8.cpu().double() @ g8.cpu().double().t()).to(torch.int64)
    assert acc.abs().max() < 2 ** 24
    sc = (acc.float() * qs.cpu()[:, None]) * gs.cpu()[None, :]
    if exclude_self:
        sc.fill_diagonal_(-float("inf"))
    s, i = torch.sort(sc, dim=1, descending=True, stable=True)
    return s[:, :k], i[:, :k].int()


@pytest.mark.parametrize("normalize", [True, False])
def test_quantizer_equals_its_definition(normalize):
    from pets_face_recognition_amd.match import quantize_rows
    g = torch.Generator().manual_seed(1)
    for D in (512, 200, 64):
        x = torch.randn(40, D, generator=g) * torch.rand(40, 1, generator=g) * 3
        x[3] = 0.0                                           # zero row
        x[5] *= 1e-20 / x[5].norm()                          # tiny and huge norms
        x[7] *= 1e6 / x[7].norm()
        x[9, :] = 0.0
        x[9, 1] = -2.5                                       # one non-zero element: exactly ±127
        q8, s, xf = quantize_rows(x.to(DEV), normalize=normalize, return_rows=True)
        Dp = (D + 127) // 128 * 128
        assert q8.shape == (40, Dp) and q8.dtype == I8 and s.shape == (40,) and xf.shape == (40, D)
        if not normalize:
            assert torch.equal(xf.cpu(), x)
        else:
            assert torch.allclose(xf.cpu(), torch.nn.functional.normalize(x, dim=1, eps=1e-12), rtol=1e-5, atol=1e-7)
        hq, hs = _quantize_host(xf)
        assert torch.equal(q8[:, :D].cpu(), hq), D
        assert torch.equal(s.cpu(), hs), D
        assert (q8[:, D:] == 0).all()                        # padding columns
        assert (q8[3] == 0).all() and s[3].item() == 0.0
        assert q8[9, 1].item() == -127 and s[9].item() > 0
        assert (q8[5] != 0).any() and (q8[7] != 0).any()
        assert q8[:, :D].abs().amax(dim=1)[[0, 1, 2, 5, 7]].eq(127).all()


@pytest.mark.parametrize("exclude_self", [False, True])
def test_selection_scores_are_exact(exclude_self):
    """rescore=False returns the top-k by the selection score: equal, bit for bit, to the host restatement, for one unfused chunk and for
    the seed + fused-filter schedule (the filter's epilogue scores and the materialised chunk's are the same bits, and no score above a
    threshold is dropped)."""
    from pets_face_recognition_amd.match import cosine_topk, quantize_rows
    g = torch.Generator().manual_seed(2)
    D = 200                                                   # Dp = 256: padded rows through both kernels
    gal = torch.randn(70000, D, generator=g).to(DEV)
    qry = gal[:300].clone() if exclude_self else torch.randn(300, D, generator=g).to(DEV)
    q8, qs = quantize_rows(qry)
    g8, gs = quantize_rows(gal)
    for k in (1, 20, 100):
        hs, hi = _selection_host(q8, qs, g8, gs, k, exclude_self)   # (exclude_self: the queries are gallery rows 0..299)
        for sched in (dict(chunk=70000), dict(chunk=16384, seed_cols=4096)):
            sc, idx = cosine_topk(qry, gal, k, compute_dtype=I8, rescore=False, exclude_self=exclude_self, **sched)
            torch.cuda.synchronize()
            assert torch.equal(idx.cpu(), hi), (k, sched)
            assert torch.equal(sc.cpu(), hs), (k, sched)


def test_schedules_agree_and_overflow_fallback():
    from oracle import match_ref
    from pets_face_recognition_amd.match import cosine_topk, quantize_rows
    g = torch.Generator().manual_seed(21)
    emb = torch.randn(700, 512, generator=g).to(DEV)
    for rescore in (False, True):
        a = cosine_topk(emb, emb, 50, compute_dtype=I8, chunk=256, exclude_self=True, fused_filter=True, rescore=rescore)
        b = cosine_topk(emb, emb, 50, compute_dtype=I8, chunk=256, exclude_self=True, fused_filter=False, rescore=rescore)
        assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0]), rescore
        assert not (a[1].cpu().long() == torch.arange(700)[:, None]).any()
    # ascending gallery (score vs q0 strictly increasing with the row): the candidate buffer overflows, the match is redone unfused
    q0 = torch.nn.functional.normalize(torch.randn(1, 512, generator=g), dim=1)
    r = torch.randn(1, 512, generator=g)
    r = torch.nn.functional.normalize(r - (r * q0).sum() * q0, dim=1)
    th = torch.linspace(1.5, 0.05, 9000)[:, None]
    gal = torch.cos(th) * q0 + torch.sin(th) * r
    qs = q0.repeat(3, 1)
    sel_f = cosine_topk(qs.to(DEV), gal.to(DEV), 10, compute_dtype=I8, chunk=4096, fused_filter=True, rescore=False)
    sel_u = cosine_topk(qs.to(DEV), gal.to(DEV), 10, compute_dtype=I8, chunk=4096, fused_filter=False, rescore=False)
    q8, s8 = quantize_rows(qs.to(DEV))
    g8, t8 = quantize_rows(gal.to(DEV))
    hs, hi = _selection_host(q8, s8, g8, t8, 10)
    for sc, idx in (sel_f, sel_u):
        assert torch.equal(idx.cpu(), hi) and torch.equal(sc.cpu(), hs)
    sc, idx = cosine_topk(qs.to(DEV), gal.to(DEV), 10, compute_dtype=I8, chunk=4096, fused_filter=True)
    rs, ri = match_ref.topk_query_gallery(qs, gal, 10)
    assert idx.cpu().long().tolist() == ri.tolist()
    assert torch.allclose(sc.cpu(), rs, rtol=1e-4, atol=1e-5)


def test_default_certified_path_equals_f32_and_bf16():
    from test_match_gpu import _sets_equal_up_to_fp64_near_ties
    from pets_face_recognition_amd import match
    g = torch.Generator().manual_seed(4)
    D, K = 128, 100
    gal = torch.randn(70000, D, generator=g)
    qry = torch.randn(300, D, generator=g)
    for chunk in (131072, 16384):
        sc, idx = match.cosine_topk(qry.to(DEV), gal.to(DEV), K, compute_dtype=I8, chunk=chunk)
        st = dict(match.last_match_stats)
        assert st["queries"] == 300 and st["candidates"] == K + match._I8_SLACK, st
        assert st["widened"] == 0 and st["exact"] == 0, st
        assert 1e-4 < st["max_selection_error"] < 1e-2, st
        rs, ri = match.cosine_topk(qry.to(DEV), gal.to(DEV), K, compute_dtype=torch.float32, chunk=chunk)
        assert _sets_equal_up_to_fp64_near_ties(idx.cpu(), ri.cpu(), qry, gal, K) == 0
        assert torch.allclose(sc, rs, rtol=0, atol=3e-6)
        bs, bi = match.cosine_topk(qry.to(DEV), gal.to(DEV), K, compute_dtype=torch.bfloat16, chunk=chunk)
        assert torch.equal(idx, bi) and torch.equal(sc, bs)


@pytest.mark.parametrize("chunk", [65536, 16384])
def test_certificate_flags_the_dense_queries(chunk):
    """near-copies of one direction (fp32 scores 1e-6 apart, int8 selection errors ~1e-3): the certificate flags exactly the dense queries,
    the fp32 re-match returns the f32 path's answer; an uncertified short int8 list loses members of those sets."""
    from test_match_gpu import _sets_equal_up_to_fp64_near_ties
    from pets_face_recognition_amd import match
    g = torch.Generator().manual_seed(11)
    D, K = 128, 50
    base = torch.randn(D, generator=g)
    dense = base[None, :] + 0.02 * torch.randn(6000, D, generator=g)
    gal = torch.cat([dense, torch.randn(54000, D, generator=g)])[torch.randperm(60000, generator=g)]
    q_dense = base[None, :] + 0.02 * torch.randn(6, D, generator=g)
    q_far = torch.randn(40, D, generator=g)
    qry = torch.cat([q_far[:20], q_dense, q_far[20:]])
    rs, ri = match.cosine_topk(qry.to(DEV), gal.to(DEV), K, compute_dtype=torch.float32, chunk=chunk)
    sc, idx = match.cosine_topk(qry.to(DEV), gal.to(DEV), K, compute_dtype=I8, chunk=chunk)
    st = dict(match.last_match_stats)
    assert st["queries"] == 46 and st["candidates"] == K + match._I8_SLACK
    assert st["widened"] == 6 and st["exact"] == 6, st
    assert 1e-4 < st["max_selection_error"] < 2e-2, st
    assert _sets_equal_up_to_fp64_near_ties(idx.cpu(), ri.cpu(), qry, gal, K) == 0
    assert torch.allclose(sc, rs, rtol=0, atol=3e-6)
    _, i_unc = match.cosine_topk(qry.to(DEV), gal.to(DEV), K, compute_dtype=I8, chunk=chunk, slack=28, certify=False)
    assert _sets_equal_up_to_fp64_near_ties(i_unc.cpu()[20:26], ri.cpu()[20:26], qry[20:26], gal, K) > 0


def test_prepared_int8_handle():
    from pets_face_recognition_amd.match import cosine_topk, prepare_gallery
    from pets_face_recognition_amd._hip import PfrError
    g = torch.Generator().manual_seed(5)
    gal = torch.randn(70000, 128, generator=g).to(DEV)
    pg = prepare_gallery(gal, compute_dtype=I8)
    pl = prepare_gallery(gal, compute_dtype=I8, rescore=False)
    assert pg.gn.dtype == I8 and pg.qscale.shape == (70000,) and pl.gn32 is None and len(pl) == 70000
    for s in range(3):
        q = torch.randn(100 + 100 * s, 128, generator=g).to(DEV)
        s1, i1 = cosine_topk(q, gal, 20, compute_dtype=I8, chunk=16384)
        s2, i2 = cosine_topk(q, pg, 20, compute_dtype=I8, chunk=16384)
        assert torch.equal(i1, i2)
        assert torch.allclose(s1, s2, rtol=0, atol=2e-6)
        s3, i3 = cosine_topk(q, gal, 20, compute_dtype=I8, chunk=16384, rescore=False)
        s4, i4 = cosine_topk(q, pl, 20, compute_dtype=I8, chunk=16384, rescore=False)
        assert torch.equal(i3, i4) and torch.equal(s3, s4)
    with pytest.raises(PfrError):
        cosine_topk(q, pg, 20)                                # bf16 call
    with pytest.raises(PfrError):
        cosine_topk(q, pg, 20, compute_dtype=I8, rescore=False)
    with pytest.raises(PfrError):
        cosine_topk(q, prepare_gallery(gal), 20, compute_dtype=I8)
    keep = i2.clone()
    gal.copy_(torch.randn(70000, 128, generator=g))          # the caller refills its buffer
    _, i5 = cosine_topk(q, pg, 20, compute_dtype=I8, chunk=16384)
    assert torch.equal(i5, keep)
    _, i6 = cosine_topk(q, gal, 20, compute_dtype=I8, chunk=16384)
    assert not torch.equal(i6, keep)


@pytest.mark.parametrize("name", ["n256", "n400", "ties"])
def test_recall_at_k_int8_identical_to_reference(name):
    from pets_face_recognition_amd.match import recall_at_k
    G = np.load(os.path.join(GOLD, "recall.npz"))
    emb = torch.tensor(G[f"{name}_emb"]).to(DEV)
    cls = torch.tensor(G[f"{name}_classes"]).to(DEV)
    got = recall_at_k(emb, cls, (10, 100), compute_dtype=I8)
    for k in (10, 100):
        assert got[k] == G[f"{name}_recall{k}_counts"].tolist(), (k, got[k])


_SHARD_SCRIPT = """
import sys, torch, torch.distributed as dist
sys.path.insert(0, {root!r})
from pets_face_recognition_amd.match import cosine_topk, cosine_topk_sharded
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
g = torch.Generator(device="cuda").manual_seed(1)
q = torch.randn(64, 512, device="cuda", generator=g); gal = torch.randn(5000, 512, device="cuda", generator=g)
for rescore in (True, False):
    s0, i0 = cosine_topk(q, gal, 20, compute_dtype=torch.int8, rescore=rescore)
    s1, i1 = cosine_topk_sharded(q, gal, 20, 0, compute_dtype=torch.int8, rescore=rescore)
    assert torch.equal(i0.long(), i1.long()) and torch.equal(s0, s1), rescore
dist.destroy_process_group()
print("OK sharded int8")
"""


def test_sharded_int8_world1(tmp_path):
    script = tmp_path / "shard_i8.py"
    script.write_text(_SHARD_SCRIPT.format(root=ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "OK sharded int8" in r.stdout


def test_config5_int8_top100_vs_fp64_oracle_on_the_1m_gallery():
    from test_fullsize_gpu import _config5_data
    from pets_face_recognition_amd import match
    Q, G, K = 64, 1000000, 100
    qry, gal = _config5_data(Q, G)
    q64 = torch.nn.functional.normalize(qry.double().cpu(), dim=1)
    scores = torch.empty(Q, G, dtype=torch.float64)
    for lo in range(0, G, 125000):
        gc = torch.nn.functional.normalize(gal[lo:lo + 125000].double().cpu(), dim=1)
        scores[:, lo:lo + 125000] = q64 @ gc.t()
    ref_sc, ref_ix = torch.topk(scores, K + 1, dim=1)
    cut = ref_sc[:, K - 1]
    sc, idx = match.cosine_topk(qry, gal, K, compute_dtype=I8)
    print("[config 5, 64 queries, int8]", match.last_match_stats)
    idx = idx.long().cpu()
    assert (idx >= 0).all()
    nd = 0
    for q in range(Q):
        got, want = set(idx[q].tolist()), set(ref_ix[q, :K].tolist())
        for j in got ^ want:
            nd += 1
            assert abs(scores[q, j].item() - cut[q].item()) < 1e-6, (q, j, scores[q, j].item(), cut[q].item())
    assert (sc.cpu().double() - torch.gather(scores, 1, idx)).abs().max() < 5e-6
    assert nd <= 4
