"""Writes tests/golden/max_strategy.npz by RUNNING the reference's own max-strategy functions (generate_tsv.py) on synthetic ragged cards.

The functions `similarity_f`, `mean_strategy_cal_scores`, `max_strategy_cal_scores` and `calc_scores` are extracted from the reference's
generate_tsv.py by name with `ast` (as oracle/make_golden.py:ref_calc_scores does — the module imports the whole inference stack at import
time); nothing of their text is copied here.  Two things are recorded on `oracle.match_ref.calc_scores_case(seed=SEED)` (24 x 260 cards,
D = 32):
  (a) pair_scores [Q, G]: `max_strategy_cal_scores` of the head photos of every card pair where both sides have head photos (NaN elsewhere);
  (b) the rows of the reference's `calc_scores` with the name `mean_strategy_cal_scores` in its namespace bound to the reference's
      `max_strategy_cal_scores`, in the layout of tests/golden/calc_scores.npz.
The reference's calc_scores raises IndexError for a query with fewer than 10 candidates: SEED is one for which it does not, and is stored
in the file.  CPU only; run once:   python tools/make_max_strategy_golden.py /path/to/reference"""
import ast
import os
import sys
import typing
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 11


def reference_functions(ref_root):
    tree = ast.parse(open(os.path.join(ref_root, "generate_tsv.py")).read())
    want = ("similarity_f", "mean_strategy_cal_scores", "max_strategy_cal_scores", "calc_scores")
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert len(fns) == len(want), [f.name for f in fns]
    ns = {"torch": torch, "F": torch.nn.functional, "np": np, "Path": Path, "List": typing.List, "Dict": typing.Dict,
          "Any": typing.Any, "tqdm": lambda it, **kw: it}
    exec(compile(ast.Module(body=fns, type_ignores=[]), "generate_tsv.max_strategy", "exec"), ns)
    return ns


def main(ref_root):
    from oracle.match_ref import calc_scores_case
    ns = reference_functions(ref_root)
    max_scores = ns["max_strategy_cal_scores"]
    ns["mean_strategy_cal_scores"] = max_scores          # calc_scores looks the name up in its globals: it now ranks by the max strategy
    seed = SEED
    while True:
        (qh, qhs, qb, qbs, qt), (gh, ghs, gb, gbs, gt) = calc_scores_case(seed=seed)

        def db(prefix, h, hs, b, bs, t):
            return {Path(f"/cards/{prefix}{c:04d}"): {"head_vectors": [torch.from_numpy(v) for v in h[hs[c]:hs[c + 1]]],
                                                      "body_vectors": [torch.from_numpy(v) for v in b[bs[c]:bs[c + 1]]],
                                                      "type": int(t[c])} for c in range(len(t))}
        try:
            rows = ns["calc_scores"](db("q", qh, qhs, qb, qbs, qt), db("g", gh, ghs, gb, gbs, gt))
            break
        except IndexError:                               # a query with fewer than 10 candidates: the reference cannot rank this case
            seed += 1
    Q, G = len(qt), len(gt)
    pair = np.full((Q, G), np.nan, np.float64)
    for i in range(Q):
        v1 = [torch.from_numpy(v) for v in qh[qhs[i]:qhs[i + 1]]]
        for j in range(G):
            v2 = [torch.from_numpy(v) for v in gh[ghs[j]:ghs[j + 1]]]
            if v1 and v2:
                pair[i, j] = max_scores(v1, v2)
    qrow = np.array([int(r[0][1:]) for r in rows])
    ans = np.full((len(rows), 100), -1, np.int64)
    for i, r in enumerate(rows):
        a = [int(n[1:]) for n in r[4].split(",")]
        ans[i, :len(a)] = a
    out = os.path.join(ROOT, "tests", "golden", "max_strategy.npz")
    np.savez_compressed(out, seed=np.int64(seed), q_head=qh, q_head_seg=qhs, q_body=qb, q_body_seg=qbs, q_type=qt, g_head=gh, g_head_seg=ghs,
                        g_body=gb, g_body_seg=gbs, g_type=gt, pair_scores=pair, rows_query=qrow, top1=np.array([r[1] for r in rows]),
                        mean3=np.array([r[2] for r in rows]), mean10=np.array([r[3] for r in rows]), answer=ans)
    print(f"{out}: seed {seed}, {len(rows)} rows of {Q} queries, {int(np.isfinite(pair).sum())} head pairs, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
