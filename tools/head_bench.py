"""Cost of the head per criterion: SoftmaxBasedMetricLearning(nn.Identity(), 10 000, 512, arc_margin=True) at B = 256, forward + backward,
bf16 and fp32 compute, two variants per criterion interleaved round by round so that box drift hits both alike:
  fused     the module's forward: every criterion inside the one margin + criterion row kernel (losses/__init__.py:_fusable)
  fallback  the path before the criteria were fused, from its unfused pieces: the margin-logit kernels (add_margin), then for adaptive
            alpha one torch multiply and the device focal-CE kernel, for nn.CrossEntropyLoss torch's own ops over the B x C logits.
            (The default criterion has always been fused: its 'fallback' row is the same unfused chain, for scale.)
The adaptive margins (AdaFace, CurricularFace; default criterion) are two more rows; their second variant is
  torch     the head as a chain of torch ops on the same device (the modules' own CPU formulation, losses/large_margin.py, run on the
            device tensors, then FocalLoss's torch arithmetic): there is no unfused margin kernel of that kind to fall back to.
The 'magface' row (MagFace: the one head with a gradient through the embedding's length) has three interleaved variants: fused, torch
(MagFaceProduct's CPU definition run on the device, regulariser included) and adaface (the fused AdaFace head of the same shape in the
same rounds, the closest fused relative: one prepare launch, the same row kernel, no radial term).
Prints one JSON line per (criterion, dtype): median / min ms of forward + backward per variant and the peak of
torch.cuda.max_memory_allocated over one forward + backward above what was allocated before it.
  python tools/head_bench.py [--rounds 8] [--steps 20] [--warmup 10] [--only default] [--variants fused]"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, C, D = 256, 10000, 512
CRITERIA = {
    "default": (True, dict()),
    "alpha_g2": (True, dict(gamma=2, alpha=True)),
    "weight": (False, dict(weight=True)),
    "smooth0.1": (False, dict(label_smoothing=0.1)),
    "adaface": (True, dict()),
    "curricular": (True, dict()),
    "magface": (True, dict()),
}
ADAPTIVE = ("adaface", "curricular", "magface")


def _magface_torch(head, emb, label):
    """MagFaceProduct.forward_with_regulariser's CPU branch (the definition in torch ops) on device tensors -> (logits, regulariser)"""
    import math
    F = nn.functional
    c = (F.normalize(emb) @ F.normalize(head.weight).t()).clamp(-1.0, 1.0)
    a = emb.norm(dim=1).clamp(head.l_a, head.u_a)
    m = (head.u_m - head.l_m) / (head.u_a - head.l_a) * (a - head.l_a) + head.l_m
    ct = c.gather(1, label[:, None]).squeeze(1)
    phi = ct * torch.cos(m) - torch.sqrt((1.0 - ct * ct).clamp_min(0.0)) * torch.sin(m)
    target = torch.where(ct > 0, phi, ct) if head.easy_margin else torch.where(ct > torch.cos(math.pi - m), phi, ct - m * torch.sin(m))
    hot = F.one_hot(label, c.shape[1]).bool()
    return head.s * torch.where(hot, target[:, None], c), head.lambda_g * (a / head.u_a ** 2 + 1.0 / a).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", default=None, choices=list(CRITERIA))
    ap.add_argument("--variants", default="fused,fallback")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_bench.py needs an MI355X")
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    from pets_face_recognition_amd.losses._head_hip import FocalCEFunction
    dev = torch.device("cuda", 0)
    torch.manual_seed(5)
    g = torch.Generator().manual_seed(5)
    emb = torch.randn(B, D, generator=g).to(dev).requires_grad_(True)
    label = torch.randint(0, C, (B,), generator=g).to(dev)
    for name, (is_focal, kw) in CRITERIA.items():
        if args.only and name != args.only:
            continue
        margin = name if name in ADAPTIVE else None
        variants = [("torch" if margin and v == "fallback" else v) for v in args.variants.split(",")]
        if name == "magface" and "fused" in variants:
            variants.append("adaface")
        kw = dict(kw)
        if kw.get("weight"):
            kw["weight"] = 0.25 + 2.0 * torch.rand(C, generator=g)
        for dt in (torch.bfloat16, torch.float32):
            wrap = SoftmaxBasedMetricLearning(nn.Identity(), C, D, is_focal=is_focal, loss_kwargs=kw, arc_margin=True, margin=margin).to(dev)
            wrap.add_margin.compute_dtype = dt
            params = [emb] + list(wrap.parameters())
            if "adaface" in variants:
                ada = SoftmaxBasedMetricLearning(nn.Identity(), C, D, is_focal=is_focal, loss_kwargs=kw, margin="adaface").to(dev)
                ada.add_margin.compute_dtype = dt
                params += list(ada.parameters())

            def step(variant):
                for p in params:
                    p.grad = None
                if variant == "fused":
                    loss = wrap(emb, label)["loss"]
                elif variant == "adaface":
                    loss = ada(emb, label)["loss"]
                elif variant == "torch":
                    head = wrap.add_margin
                    reg = 0.0
                    if name == "magface":
                        logits, reg = _magface_torch(head, emb, label)
                    else:
                        logits = head._adaptive_logits(emb, head._cpu_cosine(emb, label), label)
                    ce = nn.functional.cross_entropy(logits, label, reduction="none")
                    loss = ((1 - torch.exp(-ce)) ** wrap.focal_loss.gamma * ce).mean() + reg
                else:
                    logits = wrap.add_margin(emb, label)
                    if is_focal and kw.get("alpha"):
                        loss = FocalCEFunction.apply(wrap.focal_loss.alpha * logits, label, float(wrap.focal_loss.gamma))
                    elif is_focal:
                        loss = wrap.focal_loss(logits, label)
                    else:
                        loss = nn.functional.cross_entropy(logits, label, weight=wrap.focal_loss.weight,
                                                           label_smoothing=wrap.focal_loss.label_smoothing)
                loss.backward()
                return loss

            res = {"criterion": name, "dtype": str(dt).split(".")[1], "B": B, "C": C, "D": D}
            for v in variants:
                for _ in range(args.warmup):
                    step(v)
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                res[f"{v}_loss"] = round(step(v).item(), 5)
                res[f"{v}_peak_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            ms = {v: [] for v in variants}
            for r in range(args.rounds):
                for v in (variants if r % 2 == 0 else variants[::-1]):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        step(v)
                    torch.cuda.synchronize()
                    ms[v].append((time.perf_counter() - t0) / args.steps * 1e3)
            for v in variants:
                res[f"{v}_median_ms"] = round(statistics.median(ms[v]), 4)
                res[f"{v}_min_ms"] = round(min(ms[v]), 4)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
