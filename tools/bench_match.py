"""BASELINE config 5: query x gallery 512-d cosine match with top-100 and candR@10/100 on one MI355X.
  python tools/bench_match.py [Q] [G] [--int8]     (defaults 10000 x 1000000)
Synthetic data per SURVEY §8d: gallery = 100k classes x 10 photos, center[class] + sigma*N(0,1), L2-normalised.
--int8 adds the int8 selection (compute_dtype=torch.int8): one-shot and prepared-handle matches, the bf16 prepared handle for comparison,
their certificate statistics and top-100 set agreement with the f32 path."""
import json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pets_face_recognition_amd.match import cosine_topk
from pets_face_recognition_amd import match as _match

INT8 = "--int8" in sys.argv
argv = [a for a in sys.argv if a != "--int8"]
Q = int(argv[1]) if len(argv) > 1 else 10000
G = int(argv[2]) if len(argv) > 2 else 1000000
D, K = 512, 100
dev = 'cuda'
g = torch.Generator(device=dev).manual_seed(123)
ncls = G // 10
centers = torch.randn(ncls, D, device=dev, generator=g)
gcls = torch.arange(ncls, device=dev).repeat_interleave(10)[:G]
perm = torch.randperm(G, device=dev, generator=g)
gcls = gcls[perm]
sigma = 3.2
gal = centers[gcls] + sigma * torch.randn(G, D, device=dev, generator=g)
qcls = torch.randint(0, ncls, (Q,), device=dev, generator=g)
qry = centers[qcls] + sigma * torch.randn(Q, D, device=dev, generator=g)
res, sets = {}, {}
legs = [("bf16+fp32 rescore", torch.bfloat16, False), ("f32", torch.float32, False)]
if INT8:
    legs += [("int8+fp32 rescore", torch.int8, False), ("int8 prepared", torch.int8, True), ("bf16 prepared", torch.bfloat16, True)]
for name, dt, prep in legs:
    gx = _match.prepare_gallery(gal, compute_dtype=dt) if prep else gal   # (a handle is built once, outside the timed calls)
    sc, idx = cosine_topk(qry, gx, K, compute_dtype=dt)           # warm-up (allocations, first launches)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):                                            # median of three single matches
        t0 = time.perf_counter()
        sc, idx = cosine_topk(qry, gx, K, compute_dtype=dt)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    del gx
    dtm = sorted(ts)[1]
    hit = gcls[idx.long().clamp_min(0)] == qcls[:, None]
    r10, r100 = hit[:, :10].any(1).float().mean().item(), hit[:, :100].any(1).float().mean().item()
    sets[name] = idx.long().sort(1).values
    res[name] = dict(seconds=round(dtm, 4), tflops=round(2.0 * Q * G * D / dtm / 1e12, 1), pairs_per_s=round(Q * G / dtm / 1e9, 2),
                     candR10=round(r10, 4), candR100=round(r100, 4), idx_checksum=int(idx.long().sum().item()),
                     certificate=dict(_match.last_match_stats) if dt != torch.float32 else None)
# the two paths return the same top-100 SET unless the fp32 scores at ranks 100 / 101 differ by less than the f32-MFMA vs
# re-score summation-order noise (checked against an fp64 ranking in tests/test_fullsize_gpu.py)
a, b = sets["bf16+fp32 rescore"], sets["f32"]
same = (a == b).all(1)
out = {"workload": f"{Q} queries x {G} gallery x {D}-d, top-{K}", "results": res,
       "identical_top100_sets_bf16_vs_f32": round(same.float().mean().item(), 6),
       "queries_with_different_sets": int((~same).sum().item())}
if INT8:
    for name in ("int8+fp32 rescore", "int8 prepared"):
        same8 = (sets[name] == b).all(1)
        out[f"identical_top100_sets_{name}_vs_f32"] = round(same8.float().mean().item(), 6)
        out[f"identical_top100_sets_{name}_vs_bf16"] = round((sets[name] == a).all(1).float().mean().item(), 6)
print(json.dumps(out))
