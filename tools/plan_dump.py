#!/usr/bin/env python
"""Dump the resolved launch lists of the engines as JSON lines, for diffing two checkouts of the host-side code.

  python tools/plan_dump.py [--out FILE] [--only resnet50|resnet50_eval|swin_t]

Covers ResNet-50 (bs 256, 224x224, bf16, training forward + backward), its BN-folded inference plan and Swin-T (bs 128,
224x224, training forward + backward).  One line per list entry: the model, the list (`fwd`, `bwd0`, `bwd1` / `bwd`), the
index, the role of csrc/pfr_plan.hip (0 main launch, 1 side launch, 2 fork, 3 side record, 4 wait, 5 hook-only wait,
6 hook stop), the C-ABI function and its arguments.  Pointer arguments (by the prototype in include/pfr_hip.h) are replaced
by "p<rank of first appearance>" (null stays 0), so that two processes that allocate at different addresses print the same
text when — and only when — they hand the library the same lists; integers and floats are verbatim.  The ranks start again
for Swin-T: it runs after the ResNet was freed, and an address the allocator hands out a second time is not the same buffer.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import pets_face_recognition_amd.models as M  # noqa: E402
from pets_face_recognition_amd._hip import lib  # noqa: E402
from pets_face_recognition_amd._hip.cplan import SIDE  # noqa: E402

POINTERS = (ctypes.c_void_p, ctypes.c_char_p)


def dump_list(out, model, name, ops, ranks, protos):
    for i, (fn, args) in enumerate(ops):
        if fn is None:
            rec = {"kind": 6, "fn": None, "args": list(args)}
        elif fn.__class__ is int and fn != SIDE:
            rec = {"kind": fn, "fn": None, "args": [int(args)]}
        else:
            kind = 0
            if fn.__class__ is int:
                kind, (fn, args) = 1, args
            types = protos[fn.__name__][1]
            vals = []
            for v, t in zip(args, types):
                if t in POINTERS:
                    vals.append(0 if not v else "p%d" % ranks.setdefault(int(v), len(ranks)))
                else:
                    vals.append(v)
            rec = {"kind": kind, "fn": fn.__name__, "args": vals}
        out.write(json.dumps({"model": model, "list": name, "i": i, **rec}) + "\n")


def last_plan(eng):
    plan = getattr(eng, "_last_plan", None) or eng._last
    return getattr(plan, "meta", plan)     # (plans that are plain dicts: checkouts before models/_plan_engine.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else sys.stdout
    dev = torch.device("cuda:0")
    protos = lib.symbols()
    ranks = {}
    gen = torch.Generator().manual_seed(5)

    def train_step(m, bs):
        x = torch.rand(bs, 3, 224, 224, generator=gen).to(dev)
        emb = m(x)
        emb.backward(torch.ones_like(emb))
        torch.cuda.synchronize()

    if args.only in (None, "resnet50", "resnet50_eval"):
        torch.manual_seed(123)
        m = M.resnet50(compute_dtype=torch.bfloat16)
        m.fc = torch.nn.Linear(m.fc.in_features, 512)
        m = m.to(dev).train()
        if args.only != "resnet50_eval":
            train_step(m, 256)
            meta = last_plan(m.hip_engine())
            for k in ("fwd", "bwd0", "bwd1"):
                dump_list(out, "resnet50", k, meta[k], ranks, protos)
        if args.only != "resnet50":
            m.eval()
            with torch.no_grad():
                m(torch.rand(256, 3, 224, 224, generator=gen).to(dev))
            torch.cuda.synchronize()
            meta = last_plan(m.hip_engine())
            assert meta.get("folded")
            dump_list(out, "resnet50_eval", "fwd", meta["fwd"], ranks, protos)
        del m, meta
        torch.cuda.empty_cache()
        ranks = {}
    if args.only in (None, "swin_t"):
        torch.manual_seed(123)
        m = M.swin_t(num_classes=512, compute_dtype=torch.bfloat16).to(dev).train()
        train_step(m, 128)
        meta = last_plan(m.hip_engine())
        for k in ("fwd", "bwd"):
            dump_list(out, "swin_t", k, meta[k], ranks, protos)
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
