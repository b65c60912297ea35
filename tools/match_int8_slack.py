"""Default slack of the certified int8 selection (match._I8_SLACK): one-shot int8 matches of the config-5 data (tools/bench_match.py)
over a range of slacks, with what the certificate did.  A slack too short sends queries to the widened and fp32 re-matches; a wide
one costs re-score reads and merge work on every query.
  python tools/match_int8_slack.py [Q] [G] [slack ...]     (defaults 10000 x 1000000, slacks 48 64 96 128 160 192)"""
import json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pets_face_recognition_amd import match

Q = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
slacks = [int(a) for a in sys.argv[3:]] or [48, 64, 96, 128, 160, 192]
D, K = 512, 100
dev = 'cuda'
g = torch.Generator(device=dev).manual_seed(123)          # (the data of tools/bench_match.py)
ncls = G // 10
centers = torch.randn(ncls, D, device=dev, generator=g)
gcls = torch.arange(ncls, device=dev).repeat_interleave(10)[:G]
perm = torch.randperm(G, device=dev, generator=g)
gcls = gcls[perm]
gal = centers[gcls] + 3.2 * torch.randn(G, D, device=dev, generator=g)
qcls = torch.randint(0, ncls, (Q,), device=dev, generator=g)
qry = centers[qcls] + 3.2 * torch.randn(Q, D, device=dev, generator=g)
_, ref = match.cosine_topk(qry, gal, K, compute_dtype=torch.float32)
ref = ref.long().sort(1).values


def timed(**kw):
    match.cosine_topk(qry, gal, K, **kw)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        sc, idx = match.cosine_topk(qry, gal, K, **kw)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[1], idx, dict(match.last_match_stats)


rows = []
for s in slacks:
    t, idx, st = timed(compute_dtype=torch.int8, slack=s)
    same = (idx.long().sort(1).values == ref).all(1).float().mean().item()
    rows.append(dict(dtype="int8", slack=s, ms=round(1e3 * t, 2), same_top100_set_as_f32=round(same, 6), **st))
    print(json.dumps(rows[-1]), flush=True)
t, idx, st = timed(compute_dtype=torch.bfloat16)
print(json.dumps(dict(dtype="bfloat16", slack="default", ms=round(1e3 * t, 2), **st)), flush=True)
