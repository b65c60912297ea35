"""SwinEngine — executes the Swin-T/S/B/L feature extractor (forward, backward) on the gfx950 kernels.

Counterpart of /root/reference/models/swin.py:196-225 (`SwinTransformer.forward`) + autograd for BASELINE config 4.
Same design as models/_fe_engine.FEEngine: flat fp32 master / gradient buffers (the module's nn.Parameters become views,
state-dict names unchanged), compute-dtype shadow, one pre-built plan of C-ABI calls per input shape; the plan runtime (plan
cache, resolve, replay on two streams, autograd wrapper) is models/_plan_engine.PlanEngine, build_plan emits through its
PlanBuilder (backward buffer pool, side-stream forks and joins, deferred column sums) and the Linear / LayerNorm emitters of
models/_plan_layers.py.

Mapping (tokens are kept NHWC = [B, H, W, C] end to end; the reference's NCHW↔NHWC permutes between stages vanish):
  PatchMerging (Unfold + Linear, swin.py:155-167)  → stride-f conv on NHWC (weights re-laid out per step)
  LayerNorm / GELU / windowed attention            → csrc/pfr_swin.hip
  to_qkv / to_out / MLP / head Linear              → pfr_conv2d_fwd (GEMM, bias and residual-add fused in the epilogue),
                                                     pfr_conv2d_wgrad, data gradient through pfr_conv2d_fwd
  cyclic shift, window partition, masks            → addressing / analytic mask inside the attention kernel
"""
import struct

import torch

from .._hip import lib, PfrError
from .._hip.cplan import SIDE
from ._plan_engine import PlanEngine, PlanBuilder, Plan, engine_forward
from ._plan_layers import gemm, dgrad_lin, ln_fwd, ln_bwd, bias_grad


class _Lin:
    pass


class _LN:
    pass


class SwinEngine(PlanEngine):
    max_plans = 6

    def __init__(self, model, device, compute_dtype=None):
        super().__init__(model, device, compute_dtype)
        self.fuse_gelu = True
        self.ln_dxsum = True   # bias gradients from the LayerNorm-backward pass that produced their input
        self._adopt(model)

    # ------------------------------------------------------------------------------------------ parameters
    def _adopt(self, model):
        dev = self.device
        offs = self._adopt_flat([(n, p) for n, p in model.named_parameters() if p.requires_grad])
        for n, p in model.named_parameters():          # frozen masks just move to the device
            if not p.requires_grad:
                p.data = p.data.to(dev)

        def lin(prefix, m, conv_f=None, cin=None):
            r = _Lin()
            r.out, r.inp = m.out_features, m.in_features
            r.off = offs[prefix + ".weight"]
            r.g = self.grad[r.off:r.off + r.out * r.inp]
            if m.bias is not None:
                bo = offs[prefix + ".bias"]
                r.bias = self.master[bo:bo + r.out]
                r.dbias = self.grad[bo:bo + r.out]
            else:
                r.bias = r.dbias = None
            r.f = conv_f
            if conv_f is None:
                r.w = self.shadow[r.off:r.off + r.out * r.inp]                       # [out][in] = [out,1,1,in]
                r.wt = torch.zeros(r.inp * r.out, dtype=self.dtype, device=dev)     # [in,1,1,out]
                r.cin = r.cinp = r.inp
            else:                                                                    # patch merging as a conv
                r.cin = cin
                r.cinp = (cin + self.kp - 1) // self.kp * self.kp
                kk = conv_f * conv_f * r.cinp
                r.w = torch.zeros(r.out * kk, dtype=self.dtype, device=dev)          # [out][f][f][cinp]
                r.wt = torch.zeros(r.out * kk, dtype=self.dtype, device=dev)         # [cinp][f][f][out]
                r.g_conv = torch.zeros(r.out * kk, dtype=torch.float32, device=dev)
            return r

        def ln(prefix, m):
            r = _LN()
            r.C, r.eps = m.normalized_shape[0], m.eps
            wo, bo = offs[prefix + ".weight"], offs[prefix + ".bias"]
            r.gamma, r.beta = self.master[wo:wo + r.C], self.master[bo:bo + r.C]
            r.dgamma, r.dbeta = self.grad[wo:wo + r.C], self.grad[bo:bo + r.C]
            return r

        self.stages = []
        cin = model.stage1.patch_partition.linear.in_features // (model.stage1.patch_partition.downscaling_factor ** 2)
        self.in_channels = cin
        for si in range(1, 5):
            st = getattr(model, f"stage{si}")
            pm = st.patch_partition
            rec = {"pm": lin(f"stage{si}.patch_partition.linear", pm.linear, conv_f=pm.downscaling_factor, cin=cin),
                   "f": pm.downscaling_factor, "blocks": [], "off": offs[f"stage{si}.patch_partition.linear.weight"]}
            for li, pair in enumerate(st.layers):
                for bi, blk in enumerate(pair):
                    pre = f"stage{si}.layers.{li}.{bi}"
                    att = blk.attention_block.fn.fn
                    ff = blk.mlp_block.fn.fn
                    if not att.relative_pos_embedding:
                        raise PfrError("HIP Swin path supports relative_pos_embedding=True (the reference default)")
                    b = {"ln1": ln(pre + ".attention_block.fn.norm", blk.attention_block.fn.norm),
                         "qkv": lin(pre + ".attention_block.fn.fn.to_qkv", att.to_qkv),
                         "out": lin(pre + ".attention_block.fn.fn.to_out", att.to_out),
                         "ln2": ln(pre + ".mlp_block.fn.norm", blk.mlp_block.fn.norm),
                         "fc1": lin(pre + ".mlp_block.fn.fn.net.0", ff.net[0]),
                         "fc2": lin(pre + ".mlp_block.fn.fn.net.2", ff.net[2]),
                         "heads": att.heads, "w": att.window_size, "scale": att.scale,
                         "shift": att.window_size // 2 if att.shifted else 0}
                    po = offs[pre + ".attention_block.fn.fn.pos_embedding"]
                    ntab = (2 * att.window_size - 1) ** 2
                    b["pos"] = self.master[po:po + ntab]
                    b["dpos"] = self.grad[po:po + ntab]
                    b["hd"] = att.to_qkv.out_features // (3 * att.heads)
                    b["tab"] = torch.empty(lib.pfr_window_bias_table_floats(att.window_size), dtype=torch.float32, device=dev)
                    rec["blocks"].append(b)
            self.stages.append(rec)
            cin = pm.linear.out_features
        self.head_ln = ln("mlp_head.0", model.mlp_head[0])
        self.head_fc = lin("mlp_head.1", model.mlp_head[1])
        self.emb_dim = self.head_fc.out
        self.cp = self.stages[0]["pm"].cinp
        torch.cuda.synchronize(dev)

    def _all_lins(self):
        for st in self.stages:
            yield st["pm"]
            for b in st["blocks"]:
                for k in ("qkv", "out", "fc1", "fc2"):
                    yield b[k]
        yield self.head_fc

    def refresh_weights(self, stream, for_backward=True):
        if self.dtype != torch.float32:
            lib.pfr_cast(self.master.data_ptr(), 0, self.shadow.data_ptr(), self.did, self.n_flat, stream)
        for r in self._all_lins():
            if r.f is not None:   # Unfold order (c, kh, kw) → conv layout [out][kh][kw][c(padded)]
                lib.pfr_nchw_to_nhwc(self.master.data_ptr() + 4 * r.off, r.w.data_ptr(), self.did, r.out, r.cin, r.f * r.f, 1,
                                     r.cinp, stream)
        if for_backward:
            self._refresh_dgrad_layouts(stream)

    def _wt_records(self):
        for r in self._all_lins():
            if r.f is None:
                yield (r.w.data_ptr(), r.wt.data_ptr(), r.out, 1, 1, r.inp)
            elif r is not self.stages[0]["pm"]:      # (the first patch merging has no data gradient)
                yield (r.w.data_ptr(), r.wt.data_ptr(), r.out, r.f, r.f, r.cinp)

    # ------------------------------------------------------------------------------------------ plan
    def build_plan(self, N, H, W, with_backward):
        T, dev, did = self.dtype, self.device, self.did
        plan = Plan()
        pb = PlanBuilder(plan, T, dev, did, self.pool_depth)
        A, fwd, bwd = pb.A, pb.fwd, pb.bwd
        tab_recs = []

        x_nhwc = A((N, H, W, self.cp))
        cur, cshape = x_nhwc, (N, H, W, self.cp)
        saved = []
        for st in self.stages:
            f, pm = st["f"], st["pm"]
            Nn, Hh, Ww, Cc = cshape
            OH, OW = Hh // f, Ww // f
            rows = N * OH * OW
            C = pm.out
            t = A((N, OH, OW, C))
            fwd.append((lib.pfr_conv2d_fwd, (cur.data_ptr(), pm.w.data_ptr(), t.data_ptr(), did, did, N, Hh, Ww, Cc, C, f, f, f, 0,
                                             0, OH, OW, C, pm.bias.data_ptr() if pm.bias is not None else 0, 0, 0, 0, 0, 0, 0, 0)))
            srec = {"in": cur, "inshape": cshape, "t": t, "shape": (N, OH, OW, C), "blocks": []}
            x = t
            for b in st["blocks"]:
                ln1, mu1, rs1 = ln_fwd(pb, x, b["ln1"], rows, C)
                qkv = A((rows, 3 * C))
                gemm(pb, ln1, rows, C, b["qkv"], qkv)
                att = A((rows, C))
                tab_recs.append((b["pos"].data_ptr(), b["tab"].data_ptr(), b["w"], b["shift"]))
                fwd.append((lib.pfr_window_attn_fwd, (qkv.data_ptr(), b["tab"].data_ptr(), att.data_ptr(), did, N, OH, OW,
                                                      b["heads"], b["hd"], b["w"], b["shift"], float(b["scale"]))))
                y = A((rows, C))
                gemm(pb, att, rows, C, b["out"], y, residual=x)
                ln2, mu2, rs2 = ln_fwd(pb, y, b["ln2"], rows, C)
                h1 = A((rows, 4 * C))
                h2 = A((rows, 4 * C))
                if self.fuse_gelu:   # GELU in the fc1 GEMM's epilogue (writes the pre-activation h1 and h2 = gelu(h1))
                    fwd.append((lib.pfr_gemm_act, (ln2.data_ptr(), b["fc1"].w.data_ptr(), h2.data_ptr(), did, rows, C, 4 * C,
                                                   b["fc1"].bias.data_ptr(), 2, h1.data_ptr())))
                else:
                    gemm(pb, ln2, rows, C, b["fc1"], h1)
                    fwd.append((lib.pfr_gelu_fwd, (h1.data_ptr(), h2.data_ptr(), did, rows * 4 * C)))
                z = A((rows, C))
                gemm(pb, h2, rows, 4 * C, b["fc2"], z, residual=y)
                srec["blocks"].append(dict(x=x, ln1=ln1, mu1=mu1, rs1=rs1, qkv=qkv, att=att, y=y, ln2=ln2, mu2=mu2, rs2=rs2,
                                           h1=h1, h2=h2, z=z))
                x = z
            saved.append(srec)
            cur, cshape = x, (N, OH, OW, C)
        Nn, Hh, Ww, Cf = cshape
        pooled = A((N, Cf))
        fwd.append((lib.pfr_avgpool_fwd, (cur.data_ptr(), pooled.data_ptr(), did, N, Hh * Ww, Cf)))
        hln, hmu, hrs = ln_fwd(pb, pooled, self.head_ln, N, Cf)
        emb = A((N, self.emb_dim), torch.float32)
        gemm(pb, hln, N, Cf, self.head_fc, emb)
        # the bias(+mask) tables of every attention block in one launch at the head of the forward pass (their inputs, the relative-position
        # tables, only change in the optimiser step)
        tabd = plan.keep(torch.frombuffer(bytearray(b"".join(struct.pack("<QQii", *r) for r in tab_recs)), dtype=torch.uint8).to(dev))
        fwd.insert(0, (lib.pfr_window_bias_table_batch, (tabd.data_ptr(), len(tab_recs))))
        plan.ops = fwd
        plan.meta.update(x_nhwc=x_nhwc, emb=emb, n_fwd=len(fwd))
        if not with_backward:
            return plan

        # ================================================================= backward (stream roles, buffer pool: PlanBuilder)
        G, release, side, wgrad, colsum, pend_cs = pb.G, pb.release, pb.side, pb.wgrad, pb.colsum, pb.pend_cs
        demb = A((N, self.emb_dim))
        plan.meta["demb"] = demb
        hf = self.head_fc
        if hf.dbias is not None:
            colsum(demb, N, hf.out, hf.dbias)
        wgrad(hln, (N, 1, 1, Cf), demb, (N, 1, 1, hf.out), 1, 1, 0, hf.g)
        dhln = G((N, Cf))
        dgrad_lin(pb, demb, N, hf, dhln)
        dpooled = G((N, Cf))
        ln_bwd(pb, dhln, pooled, hmu, hrs, self.head_ln, None, dpooled, N, Cf, dxsum=self.ln_dxsum)
        dz_sum = None   # column sums of dz left by the pass that produced it (None: avgpool / patch-merging data gradient)
        release(dhln)
        dz = G(cshape)
        bwd.append((lib.pfr_avgpool_bwd, (dpooled.data_ptr(), dz.data_ptr(), did, N, Hh * Ww, Cf)))
        release(dpooled)
        bwd.append((None, (self.offs["mlp_head.0.weight"],)))
        for si in range(len(self.stages) - 1, -1, -1):
            st, srec = self.stages[si], saved[si]
            Nn, OH, OW, C = srec["shape"]
            rows = N * OH * OW
            for b, sv in zip(reversed(st["blocks"]), reversed(srec["blocks"])):
                # ---- MLP branch: z = fc2(gelu(fc1(ln2(y)))) + y
                bias_grad(pb, dz.view(rows, C), rows, C, b["fc2"].dbias, dz_sum)
                wgrad(sv["h2"], (rows, 1, 1, 4 * C), dz, (rows, 1, 1, C), 1, 1, 0, b["fc2"].g)
                dh2 = G((rows, 4 * C))
                if self.fuse_gelu:   # dh1 = (dz·W2) ∘ gelu'(h1) in the data-gradient GEMM's epilogue
                    # ... which also leaves the per-m-tile column means of dh1: fc1's bias gradient = sum_t rows_t * mean_t, merged
                    # with the other deferred column sums -- no second pass over the widest gradient tensor of the block
                    nsum = lib.pfr_gemm_act_colsum_parts(rows, C, 4 * C, did)
                    if nsum > 0:     # streaming Linear kernel (csrc/pfr_slin.hip): plain column sums per row range
                        stp = A((nsum, 4 * C), torch.float32)
                        bwd.append((lib.pfr_gemm_act_colsums, (dz.data_ptr(), b["fc2"].wt.data_ptr(), dh2.data_ptr(), did, rows, C, 4 * C,
                                                               sv["h1"].data_ptr(), stp.data_ptr())))
                        pend_cs.append((stp, b["fc1"].dbias, nsum, 4 * C, 0, 0))
                    else:
                        mt = lib.pfr_gemm_act_mtile(rows, C, 4 * C, did)
                        nt = (rows + mt - 1) // mt
                        stp = A((nt, 2, 4 * C), torch.float32)
                        bwd.append((lib.pfr_gemm_act_colstats, (dz.data_ptr(), b["fc2"].wt.data_ptr(), dh2.data_ptr(), did, rows, C, 4 * C, 0,
                                                                3, sv["h1"].data_ptr(), stp.data_ptr())))
                        pend_cs.append((stp, b["fc1"].dbias, nt, 4 * C, mt, rows))
                else:
                    dgrad_lin(pb, dz, rows, b["fc2"], dh2)
                    bwd.append((lib.pfr_gelu_bwd, (sv["h1"].data_ptr(), dh2.data_ptr(), dh2.data_ptr(), did, rows * 4 * C)))
                    colsum(dh2, rows, 4 * C, b["fc1"].dbias)
                wgrad(sv["ln2"], (rows, 1, 1, C), dh2, (rows, 1, 1, 4 * C), 1, 1, 0, b["fc1"].g)
                dln2 = G((rows, C))
                dgrad_lin(pb, dh2, rows, b["fc1"], dln2)
                release(dh2)
                dy = G((rows, C))
                dy_sum = ln_bwd(pb, dln2, sv["y"], sv["mu2"], sv["rs2"], b["ln2"], dz, dy, rows, C, want_sum=True, dxsum=self.ln_dxsum)
                release(dln2)
                release(dz)
                # ---- attention branch: y = to_out(attn(to_qkv(ln1(x)))) + x
                bias_grad(pb, dy, rows, C, b["out"].dbias, dy_sum)
                wgrad(sv["att"], (rows, 1, 1, C), dy, (rows, 1, 1, C), 1, 1, 0, b["out"].g)
                datt = G((rows, C))
                dgrad_lin(pb, dy, rows, b["out"], datt)
                dqkv = G((rows, 3 * C))
                nblk = N * (OH // b["w"]) * (OW // b["w"]) * b["heads"]
                ntab = (2 * b["w"] - 1) ** 2
                dpart = G((nblk, ntab), torch.float32)
                bwd.append((lib.pfr_window_attn_bwd, (sv["qkv"].data_ptr(), b["tab"].data_ptr(), datt.data_ptr(), dqkv.data_ptr(),
                                                      dpart.data_ptr(), did, N, OH, OW, b["heads"], b["hd"], b["w"], b["shift"],
                                                      float(b["scale"]))))
                colsum(dpart, nblk, ntab, b["dpos"], 0)
                release(dpart)
                release(datt)
                wgrad(sv["ln1"], (rows, 1, 1, C), dqkv, (rows, 1, 1, 3 * C), 1, 1, 0, b["qkv"].g)
                dln1 = G((rows, C))
                dgrad_lin(pb, dqkv, rows, b["qkv"], dln1)
                release(dqkv)
                dx = G((rows, C))
                dz_sum = ln_bwd(pb, dln1, sv["x"], sv["mu1"], sv["rs1"], b["ln1"], dy, dx, rows, C, want_sum=True, dxsum=self.ln_dxsum)
                release(dln1)
                release(dy)
                dz = dx
            # ---- patch merging (stride-f conv): bias, weight gradient (conv layout → Unfold layout), data gradient
            pm, f = st["pm"], st["f"]
            Ni, Hi, Wi, Ci = srec["inshape"]
            if pm.dbias is not None:
                bias_grad(pb, dz, rows, C, pm.dbias, dz_sum)
            g_conv = pm.g_conv
            wgrad(srec["in"], (Ni, Hi, Wi, Ci), dz, (N, OH, OW, C), f, f, 0, g_conv)
            side((SIDE, (lib.pfr_nhwc_to_nchw_f32, (g_conv.data_ptr(), pm.g.data_ptr(), pm.out, pm.cin, f * f, pm.cinp, 0))))
            if si > 0:
                din = G((Ni, Hi, Wi, Ci))
                bwd.append((lib.pfr_conv2d_fwd, (dz.data_ptr(), pm.wt.data_ptr(), din.data_ptr(), did, did, N, OH, OW, C, Ci, f, f, 1,
                                                 f - 1, {2: 1, 4: 2}[f], Hi, Wi, Ci, 0, 0, 0, 0, 0, 0, 0, 0)))
                release(dz)
                dz = din
            dz_sum = None
            pb.mark(st["off"], last=si == 0)
        return pb.finish(self)

    def forward(self, x, with_backward, ticket=None):
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise PfrError(f"expected NCHW input with {self.in_channels} channels, got {tuple(x.shape)}")
        x = x.float().contiguous()
        N, _, H, W = x.shape
        return self._forward_plan(x, N, H, W, with_backward, with_backward=with_backward, ticket=ticket)


swin_forward = engine_forward
