#!/usr/bin/env python
"""Dump the resolved launch lists of the engines as JSON lines, for diffing two checkouts of the host-side code.

  python tools/plan_dump.py [--out FILE] [--only MODEL] [--small]

Covers every backbone with an engine, each with a training forward + backward and, where the engine has an inference plan of its
own, an eval forward (`<model>_eval`: ResNet-50's BN-folded plan, the running-statistics plans of MobileNetV2 and EfficientNet-B2):

  model             default (bf16)    --small (bf16 and fp32, the smallest geometry the model's GPU tests run it at)
  resnet50          256 x 224 x 224   6 x 64 x 64
  swin_t            128 x 224 x 224   2 x 224 x 224
  convnext_tiny     128 x 224 x 224   4 x 64 x 64
  mobilenet_v2      256 x 224 x 224   4 x 64 x 64
  efficientnet_b2   128 x 224 x 224   2 x 64 x 64
  vit_b_16           64 x 224 x 224   2 x 224 x 224

Without --only the default run is ResNet-50 and Swin-T (the two-model dump this tool started as); --only takes any model above, or
`resnet50_eval`, or `all`.  --small runs all of them unless --only names one, and labels the lines `<model>.<dtype>`.

One line per list entry: the model, the list (`fwd`, `bwd0`, `bwd1` / `bwd`), the index, the role of csrc/pfr_plan.hip (0 main
launch, 1 side launch, 2 fork, 3 side record, 4 wait, 5 hook-only wait, 6 hook stop), the C-ABI function and its arguments.
Pointer arguments (by the prototype in include/pfr_hip.h) are replaced by "p<rank of first appearance>" (null stays 0), so that two
processes that allocate at different addresses print the same text when — and only when — they hand the library the same lists;
integers and floats are verbatim.  The ranks start again for every model: it runs after the one before was freed, and an address the
allocator hands out a second time is not the same buffer.
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


def _resnet50(dt):
    m = M.resnet50(compute_dtype=dt)
    m.fc = torch.nn.Linear(m.fc.in_features, 512)
    return m


def _efficientnet_b2(dt):
    m = M.efficientnet_b2(compute_dtype=dt)
    m.classifier = torch.nn.Linear(m.classifier[1].in_features, 512)     # the reference's head (no Dropout in front of it)
    return m


def _vit_b_16(dt):
    m = M.vit_b_16(compute_dtype=dt)
    m.heads = torch.nn.Linear(768, 512)
    return m


# model -> (constructor, (batch, image size), the same under --small, backward lists, has an eval plan of its own)
MODELS = {
    "resnet50": (_resnet50, (256, 224), (6, 64), ("bwd0", "bwd1"), True),
    "swin_t": (lambda dt: M.swin_t(num_classes=512, compute_dtype=dt), (128, 224), (2, 224), ("bwd",), False),
    "convnext_tiny": (lambda dt: M.convnext_tiny(num_classes=512, compute_dtype=dt), (128, 224), (4, 64), ("bwd",), False),
    "mobilenet_v2": (lambda dt: M.mobilenet_v2(num_classes=512, dropout=0, compute_dtype=dt), (256, 224), (4, 64), ("bwd",), True),
    "efficientnet_b2": (_efficientnet_b2, (128, 224), (2, 64), ("bwd",), True),
    "vit_b_16": (_vit_b_16, (64, 224), (2, 224), ("bwd",), False),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, choices=list(MODELS) + ["resnet50_eval", "all"])
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else sys.stdout
    dev = torch.device("cuda:0")
    protos = lib.symbols()
    gen = torch.Generator().manual_seed(5)
    if args.only in (None, "all"):
        names = list(MODELS) if (args.small or args.only == "all") else ["resnet50", "swin_t"]
    else:
        names = [args.only.replace("_eval", "")]
    dtypes = (("bf16", torch.bfloat16), ("fp32", torch.float32)) if args.small else (("bf16", torch.bfloat16),)

    for name in names:
        build, full, small, bwd_lists, has_eval = MODELS[name]
        bs, hw = small if args.small else full
        for dname, dt in dtypes:
            label = f"{name}.{dname}" if args.small else name
            ranks = {}
            torch.manual_seed(123)
            m = build(dt).to(dev).train()
            if args.only != "resnet50_eval":
                emb = m(torch.rand(bs, 3, hw, hw, generator=gen).to(dev))
                emb.backward(torch.ones_like(emb))
                torch.cuda.synchronize()
                meta = last_plan(m.hip_engine())
                for k in ("fwd",) + bwd_lists:
                    dump_list(out, label, k, meta[k], ranks, protos)
            if has_eval and args.only != "resnet50":
                m.eval()
                with torch.no_grad():
                    m(torch.rand(bs, 3, hw, hw, generator=gen).to(dev))
                torch.cuda.synchronize()
                meta = last_plan(m.hip_engine())
                assert name != "resnet50" or meta.get("folded")
                dump_list(out, label.replace(name, name + "_eval"), "fwd", meta["fwd"], ranks, protos)
            del m, meta
            torch.cuda.empty_cache()
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
