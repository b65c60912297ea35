"""ViTEngine — executes the Vision Transformer feature extractor (forward, backward) on the gfx950 kernels.

Same design as models/_swin_engine.SwinEngine: flat fp32 master / gradient buffers (the module's nn.Parameters become views,
torchvision's state-dict names unchanged), compute-dtype shadow, one pre-built plan of C-ABI calls per input shape; the plan runtime
is models/_plan_engine.PlanEngine.  Tokens are [B, S, D] rows end to end.

Mapping (models/vit.py):
  conv_proj (patch x patch, stride patch)          → pfr_conv2d_fwd on NHWC (weights re-laid out per step), pfr_conv2d_wgrad; no data gradient
  [class_token; patches] + pos_embedding           → pfr_vit_tokens_fwd / pfr_vit_tokens_bwd (csrc/pfr_mha.hip)
  LayerNorm                                        → pfr_layernorm_fwd / pfr_layernorm_bwd_dxsum
  in_proj / out_proj / mlp.3 / heads               → pfr_conv2d_fwd (GEMM, bias and residual-add fused in the epilogue), pfr_conv2d_wgrad
  mlp.0 + GELU                                     → pfr_gemm_act (GELU in the epilogue; its backward in the data-gradient GEMM's)
  attention over the whole sequence                → pfr_mha_fwd / pfr_mha_bwd (csrc/pfr_mha.hip)
  encoder.ln on the class-token rows, heads        → pfr_vit_cls_fwd / pfr_vit_cls_bwd, pfr_layernorm_*, pfr_conv2d_fwd
"""
import struct

import torch
import torch.nn as nn

from .._hip import lib, dtype_id, PfrError
from .._hip.cplan import SIDE, FORK, SREC, WAIT, MWAIT
from ._plan_engine import PlanEngine, Plan, engine_forward, flat_offsets


class _Rec:
    pass


def _head_linear(heads):
    """(parameter prefix, Linear) of `heads`: a bare Linear, or a Sequential whose only Linear is its last module"""
    if isinstance(heads, nn.Linear):
        return "heads", heads
    if isinstance(heads, nn.Sequential) and len(heads):
        names = list(heads._modules)
        last = heads[len(heads) - 1]
        rest = [heads._modules[n] for n in names[:-1]]
        if isinstance(last, nn.Linear) and all(isinstance(m, (nn.Identity, nn.Dropout)) and not list(m.parameters()) for m in rest) \
                and not any(isinstance(m, nn.Dropout) and m.p > 0 for m in rest):
            return f"heads.{names[-1]}", last
    raise PfrError("HIP ViT path needs `heads` to be a Linear, or a Sequential whose only Linear is its last module")


class ViTEngine(PlanEngine):
    max_plans = 6
    mark_every = 4    # encoder layers per grad-ready mark (DDP bucket boundary) and batched column-sum merge

    def __init__(self, model, device, compute_dtype=None):
        super().__init__(model, device, compute_dtype)
        self.pool_depth = 48   # see SwinEngine: backward buffers per class before one a side-stream op still reads is re-used
        self._adopt(model)

    # ------------------------------------------------------------------------------------------ parameters
    def _adopt(self, model):
        dev = self.device
        head_name, head = _head_linear(model.heads)
        if head.bias is None:
            raise PfrError("HIP ViT path: the embedding Linear has a bias")
        self.heads_n, self.hd = model.num_heads, model.hidden_dim // model.num_heads
        self.D, self.S, self.patch, self.image_size = model.hidden_dim, model.seq_length, model.patch_size, model.image_size
        if not lib.pfr_mha_supported(self.did, self.S, self.heads_n, self.hd):
            raise PfrError(f"HIP ViT path: no attention kernel for head_dim {self.hd}, {self.S} tokens (pfr_mha_supported: head_dim 64, "
                           f"at most 257 tokens)")
        if self.D % self.kp:
            raise PfrError(f"HIP ViT path: hidden_dim {self.D} must be a multiple of {self.kp} in {self.dtype}")
        self._p_drop = max(model.dropout, model.attention_dropout)
        named = list(model.named_parameters())
        if not all(p.requires_grad for _, p in named):
            raise PfrError("HIP ViT path trains every parameter (no frozen layers)")
        offs, total = flat_offsets(named)
        self.n_flat = total
        self.master = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.shadow = self.master if self.dtype == torch.float32 else torch.zeros(total, dtype=self.dtype, device=dev)
        self.offs = offs
        self._views = {}
        self.param_list = []
        for name, p in named:
            o, n = offs[name], p.numel()
            mv = self.master[o:o + n].view(p.shape)
            mv.copy_(p.data.detach().to(dev))
            p.data = mv
            p.grad = None
            self._views[name] = (p, self.grad[o:o + n].view(p.shape))
            self.param_list.append(p)
        self.first_param = named[0][1]

        def vec(name, n):
            o = offs[name]
            return self.master[o:o + n], self.grad[o:o + n]

        def lin(wname, bname, out, inp):
            r = _Rec()
            r.out, r.inp, r.f = out, inp, None
            r.off = offs[wname]
            r.g = self.grad[r.off:r.off + out * inp]
            r.bias, r.dbias = vec(bname, out)
            r.w = self.shadow[r.off:r.off + out * inp]                           # [out][in] = [out,1,1,in]
            r.wt = torch.zeros(inp * out, dtype=self.dtype, device=dev)         # [in,1,1,out]
            return r

        def ln(prefix, m):
            r = _Rec()
            r.C, r.eps = m.normalized_shape[0], m.eps
            r.gamma, r.dgamma = vec(prefix + ".weight", r.C)
            r.beta, r.dbeta = vec(prefix + ".bias", r.C)
            return r

        cv = _Rec()   # conv_proj: [D][3][p][p] parameter ↔ [D][p][p][3 padded] conv layout
        m = model.conv_proj
        cv.out, cv.cin, cv.f = m.out_channels, m.in_channels, m.kernel_size[0]
        cv.cinp = (cv.cin + self.kp - 1) // self.kp * self.kp
        cv.off = offs["conv_proj.weight"]
        kk = cv.f * cv.f * cv.cinp
        cv.g = self.grad[cv.off:cv.off + cv.out * cv.cin * cv.f * cv.f]
        cv.bias, cv.dbias = vec("conv_proj.bias", cv.out)
        cv.w = torch.zeros(cv.out * kk, dtype=self.dtype, device=dev)
        cv.g_conv = torch.zeros(cv.out * kk, dtype=torch.float32, device=dev)
        self.conv = cv
        self.cls, self.dcls = vec("class_token", self.D)
        self.pos, self.dpos = vec("encoder.pos_embedding", self.S * self.D)
        self.layers = []
        for name, blk in model.encoder.layers.named_children():
            pre = f"encoder.layers.{name}"
            att = blk.self_attention
            if not att._qkv_same_embed_dim or att.in_proj_bias is None or att.bias_k is not None or att.add_zero_attn:
                raise PfrError(f"{pre}: the HIP ViT path runs nn.MultiheadAttention with one in_proj, biases, no bias_k / zero_attn")
            b = _Rec()
            b.off = offs[pre + ".ln_1.weight"]
            b.ln1 = ln(pre + ".ln_1", blk.ln_1)
            b.qkv = lin(pre + ".self_attention.in_proj_weight", pre + ".self_attention.in_proj_bias", 3 * self.D, self.D)
            b.out = lin(pre + ".self_attention.out_proj.weight", pre + ".self_attention.out_proj.bias", self.D, self.D)
            b.ln2 = ln(pre + ".ln_2", blk.ln_2)
            b.fc1 = lin(pre + ".mlp.0.weight", pre + ".mlp.0.bias", blk.mlp[0].out_features, self.D)
            b.fc2 = lin(pre + ".mlp.3.weight", pre + ".mlp.3.bias", self.D, blk.mlp[3].in_features)
            if not isinstance(blk.mlp[1], nn.GELU) or getattr(blk.mlp[1], "approximate", "none") != "none":
                raise PfrError(f"{pre}: the HIP ViT path runs the exact GELU")
            self.layers.append(b)
        self.head_ln = ln("encoder.ln", model.encoder.ln)
        self.head_fc = lin(head_name + ".weight", head_name + ".bias", head.out_features, head.in_features)
        self.head_off = offs["encoder.ln.weight"]
        self.emb_dim = self.head_fc.out
        self.in_channels = cv.cin
        self.cp = cv.cinp
        self.scale = 1.0 / float(self.hd) ** 0.5
        torch.cuda.synchronize(dev)

    def _all_lins(self):
        for b in self.layers:
            yield b.qkv
            yield b.out
            yield b.fc1
            yield b.fc2
        yield self.head_fc

    def refresh_weights(self, stream, for_backward=True):
        """compute-dtype shadow and the conv layout of conv_proj from the fp32 master — on every forward pass, so an optimizer step,
        swap_averaged() or a loaded checkpoint needs no call of its own"""
        if self.dtype != torch.float32:
            lib.pfr_cast(self.master.data_ptr(), 0, self.shadow.data_ptr(), self.did, self.n_flat, stream)
        r = self.conv      # [O][I][f*f] → [O][f*f][I padded]
        lib.pfr_nchw_to_nhwc(self.master.data_ptr() + 4 * r.off, r.w.data_ptr(), self.did, r.out, r.cin, r.f * r.f, 1, r.cinp, stream)
        if for_backward:
            self._refresh_dgrad_layouts(stream)

    def _wt_records(self):
        for r in self._all_lins():      # (conv_proj reads the image: no data gradient)
            yield (r.w.data_ptr(), r.wt.data_ptr(), r.out, 1, 1, r.inp)

    # ------------------------------------------------------------------------------------------ plan
    def build_plan(self, N, H, W, with_backward):
        T, dev, did = self.dtype, self.device, self.did
        D, S, heads, hd, scale = self.D, self.S, self.heads_n, self.hd, self.scale
        plan = Plan()
        fwd, bwd = [], []

        def A(shape, dtype=None):
            return plan.keep(torch.empty(shape, dtype=dtype or T, device=dev))

        def gemm(ops, x, rows, cin, r, y, residual=None):
            ops.append((lib.pfr_conv2d_fwd, (x.data_ptr(), r.w.data_ptr(), y.data_ptr(), did, dtype_id(y.dtype), rows, 1, 1, cin, r.out,
                                             1, 1, 1, 0, 0, 1, 1, r.out, r.bias.data_ptr(),
                                             0 if residual is None else residual.data_ptr(), 0, 0, 0, 0, 0, 0)))

        def ln_fwd(ops, x, lnrec, rows, C):
            y = A((rows, C)); mu = A((rows,), torch.float32); rs = A((rows,), torch.float32)
            ops.append((lib.pfr_layernorm_fwd, (x.data_ptr(), lnrec.gamma.data_ptr(), lnrec.beta.data_ptr(), y.data_ptr(), mu.data_ptr(),
                                                rs.data_ptr(), did, rows, C, float(lnrec.eps))))
            return y, mu, rs

        cv = self.conv
        f = cv.f
        OH, OW = H // f, W // f
        rows = N * S
        x_nhwc = A((N, H, W, self.cp))
        patches = A((N, OH, OW, D))
        fwd.append((lib.pfr_conv2d_fwd, (x_nhwc.data_ptr(), cv.w.data_ptr(), patches.data_ptr(), did, did, N, H, W, self.cp, D, f, f, f, 0, 0,
                                         OH, OW, D, cv.bias.data_ptr(), 0, 0, 0, 0, 0, 0, 0)))
        x = A((rows, D))
        fwd.append((lib.pfr_vit_tokens_fwd, (patches.data_ptr(), self.cls.data_ptr(), self.pos.data_ptr(), x.data_ptr(), did, N, S, D)))
        saved = []
        for b in self.layers:
            Hd = b.fc1.out
            ln1, mu1, rs1 = ln_fwd(fwd, x, b.ln1, rows, D)
            qkv = A((rows, 3 * D))
            gemm(fwd, ln1, rows, D, b.qkv, qkv)
            att = A((rows, D))
            lse = A((N, heads, S), torch.float32)
            fwd.append((lib.pfr_mha_fwd, (qkv.data_ptr(), att.data_ptr(), lse.data_ptr(), did, N, S, heads, hd, scale)))
            y = A((rows, D))
            gemm(fwd, att, rows, D, b.out, y, residual=x)
            ln2, mu2, rs2 = ln_fwd(fwd, y, b.ln2, rows, D)
            h1 = A((rows, Hd))
            h2 = A((rows, Hd))
            # GELU in the fc1 GEMM's epilogue (writes the pre-activation h1 and h2 = gelu(h1))
            fwd.append((lib.pfr_gemm_act, (ln2.data_ptr(), b.fc1.w.data_ptr(), h2.data_ptr(), did, rows, D, Hd, b.fc1.bias.data_ptr(), 2,
                                           h1.data_ptr())))
            z = A((rows, D))
            gemm(fwd, h2, rows, Hd, b.fc2, z, residual=y)
            saved.append(dict(x=x, ln1=ln1, mu1=mu1, rs1=rs1, qkv=qkv, att=att, lse=lse, y=y, ln2=ln2, mu2=mu2, rs2=rs2, h1=h1, h2=h2))
            x = z
        # encoder.ln on the class-token rows only (row 0 of every sample is all the head reads)
        ctok = A((N, D))
        fwd.append((lib.pfr_vit_cls_fwd, (x.data_ptr(), ctok.data_ptr(), did, N, S, D)))
        hln, hmu, hrs = ln_fwd(fwd, ctok, self.head_ln, N, D)
        emb = A((N, self.emb_dim), torch.float32)
        gemm(fwd, hln, N, D, self.head_fc, emb)
        plan.ops = fwd
        plan.meta.update(x_nhwc=x_nhwc, emb=emb, n_fwd=len(fwd))
        if not with_backward:
            return plan

        # ================================================================= backward
        # Weight gradients and column sums feed nothing before the optimizer: they run on the SIDE stream with the FORK / SREC / WAIT
        # roles of _hip/cplan.py, exactly as in SwinEngine.build_plan (see the comments there).
        pool = {}
        nalloc = {}
        pending = {}      # data_ptr of a pooled buffer -> last side op that reads it
        side_reads = []   # (k, data_ptr) of every side-op input
        nside = [0]
        ws_need = [0]
        pend_cs = []      # deferred final merges: (partials, out, partial rows, C, tile height | 0, rows)

        def G(shape, dtype=None):
            key = (tuple(shape), dtype or T)
            lst = pool.setdefault(key, [])
            for i, t in enumerate(lst):
                if t.data_ptr() not in pending:
                    return lst.pop(i)
            if not lst or nalloc.get(key, 0) < self.pool_depth:
                nalloc[key] = nalloc.get(key, 0) + 1
                return A(shape, dtype)
            t = lst.pop(0)
            bwd.append((WAIT, pending.pop(t.data_ptr())))
            return t

        def release(t):
            lo, hi = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
            ks = [k for k, ptr in side_reads if lo <= ptr < hi]
            if ks:
                pending[t.data_ptr()] = max(ks)
            side_reads[:] = [(k, ptr) for k, ptr in side_reads if not (lo <= ptr < hi)]
            pool.setdefault((tuple(t.shape), t.dtype), []).append(t)

        def side(ops, op, *reads):
            if ops and ops[-1][0] == SREC:
                k = ops.pop()[1]
            else:
                k = nside[0]
                nside[0] += 1
                ops.append((FORK, k))
            ops.append(op)
            ops.append((SREC, k))
            for r in reads:
                side_reads.append((k, r.data_ptr()))

        def wgrad(ops, xin, xshape, dy, dyshape, R, stride, out):
            Nq, Hq, Wq, Cq = xshape
            _, oh, ow, Co = dyshape
            KK = R * R * Cq
            splits = lib.pfr_conv2d_wgrad_splits(Nq * oh * ow, Co, KK)
            ws_need[0] = max(ws_need[0], splits * Co * KK)
            side(ops, ("wgrad", (xin.data_ptr(), dy.data_ptr(), out.data_ptr(), None, did, Nq, Hq, Wq, Cq, Co, R, R, stride, 0,
                                oh, ow, Co, 0, 0, 0, 1.0, 0)), dy)

        def dgrad_lin(ops, dy, nrows, r, dx):
            ops.append((lib.pfr_conv2d_fwd, (dy.data_ptr(), r.wt.data_ptr(), dx.data_ptr(), did, did, nrows, 1, 1, r.out, r.inp, 1,
                                             1, 1, 0, 0, 1, 1, r.inp, 0, 0, 0, 0, 0, 0, 0, 0)))

        def colsum(ops, t, nrows, C, out):
            n = lib.pfr_colsum_parts(did, nrows, C)
            if n <= 0:
                side(ops, (SIDE, (lib.pfr_colsum, (t.data_ptr(), did, nrows, C, out.data_ptr(), 0, 0))), t)
                return
            ws = A((lib.pfr_colsum_ws_floats(nrows, C),), torch.float32)
            side(ops, (SIDE, (lib.pfr_colsum_partial, (t.data_ptr(), did, nrows, C, ws.data_ptr()))), t)
            pend_cs.append((ws, out, n, C, 0, 0))

        def flush_colsums(ops):
            if not pend_cs:
                return
            raw = b"".join(struct.pack("<QQiiiiii", ws.data_ptr(), out.data_ptr(), n, C, 0, mt, rws, 0) for ws, out, n, C, mt, rws in pend_cs)
            tab = plan.keep(torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev))
            side(ops, (SIDE, (lib.pfr_colsum_final_batch, (tab.data_ptr(), len(pend_cs), max(e[3] for e in pend_cs)))))
            del pend_cs[:]

        def ln_bwd(ops, dy, xin, mu, rs, lnrec, dres, dx, nrows, C, want_sum=False):
            """→ (partials, rows of partials) of the column sums of dx when want_sum and the kernel can emit them, else None"""
            nb = lib.pfr_layernorm_bwd_blocks(nrows)
            part = A((2, nb, C), torch.float32)
            dsum = A((nb, C), torch.float32) if (want_sum and lib.pfr_layernorm_bwd_dxsum_ok(did, C)) else None
            ops.append((lib.pfr_layernorm_bwd_dxsum, (dy.data_ptr(), xin.data_ptr(), mu.data_ptr(), rs.data_ptr(), lnrec.gamma.data_ptr(),
                                                      0 if dres is None else dres.data_ptr(), dx.data_ptr(), part.data_ptr(),
                                                      0 if dsum is None else dsum.data_ptr(), did, nrows, C)))
            pend_cs.append((part[0], lnrec.dgamma, nb, C, 0, 0))
            pend_cs.append((part[1], lnrec.dbeta, nb, C, 0, 0))
            return None if dsum is None else (dsum, nb)

        def bias_grad(ops, g, nrows, C, dbias, gsum):
            if gsum is not None:
                pend_cs.append((gsum[0], dbias, gsum[1], C, 0, 0))
            else:
                colsum(ops, g, nrows, C, dbias)

        def mark(ops, off, last=False):
            flush_colsums(ops)
            if nside[0]:   # everything the side stream was given so far is final
                ops.append((WAIT if last else MWAIT, nside[0] - 1))
            ops.append((None, (off,)))

        # ---- heads, encoder.ln on the class-token rows
        demb = A((N, self.emb_dim))
        plan.meta["demb"] = demb
        hf = self.head_fc
        colsum(bwd, demb, N, hf.out, hf.dbias)
        wgrad(bwd, hln, (N, 1, 1, D), demb, (N, 1, 1, hf.out), 1, 1, hf.g)
        dhln = G((N, D))
        dgrad_lin(bwd, demb, N, hf, dhln)
        dctok = G((N, D))
        ln_bwd(bwd, dhln, ctok, hmu, hrs, self.head_ln, None, dctok, N, D)
        release(dhln)
        dz = G((rows, D))
        bwd.append((lib.pfr_vit_cls_bwd, (dctok.data_ptr(), dz.data_ptr(), did, N, S, D)))
        release(dctok)
        dz_sum = None   # column sums of dz left by the pass that produced it
        mark(bwd, self.head_off)
        for li in range(len(self.layers) - 1, -1, -1):
            b, sv = self.layers[li], saved[li]
            Hd = b.fc1.out
            # ---- MLP branch: z = fc2(gelu(fc1(ln2(y)))) + y
            bias_grad(bwd, dz, rows, D, b.fc2.dbias, dz_sum)
            wgrad(bwd, sv["h2"], (rows, 1, 1, Hd), dz, (rows, 1, 1, D), 1, 1, b.fc2.g)
            dh = G((rows, Hd))
            # dh1 = (dz·W2) ∘ gelu'(h1) in the data-gradient GEMM's epilogue, which also leaves the column sums of dh1 (fc1's bias gradient)
            nsum = lib.pfr_gemm_act_colsum_parts(rows, D, Hd, did)
            if nsum > 0:     # streaming Linear kernel: plain column sums per row range
                stp = A((nsum, Hd), torch.float32)
                bwd.append((lib.pfr_gemm_act_colsums, (dz.data_ptr(), b.fc2.wt.data_ptr(), dh.data_ptr(), did, rows, D, Hd,
                                                       sv["h1"].data_ptr(), stp.data_ptr())))
                pend_cs.append((stp, b.fc1.dbias, nsum, Hd, 0, 0))
            else:
                mt = lib.pfr_gemm_act_mtile(rows, D, Hd, did)
                nt = (rows + mt - 1) // mt
                stp = A((nt, 2, Hd), torch.float32)
                bwd.append((lib.pfr_gemm_act_colstats, (dz.data_ptr(), b.fc2.wt.data_ptr(), dh.data_ptr(), did, rows, D, Hd, 0, 3,
                                                        sv["h1"].data_ptr(), stp.data_ptr())))
                pend_cs.append((stp, b.fc1.dbias, nt, Hd, mt, rows))
            wgrad(bwd, sv["ln2"], (rows, 1, 1, D), dh, (rows, 1, 1, Hd), 1, 1, b.fc1.g)
            dln2 = G((rows, D))
            dgrad_lin(bwd, dh, rows, b.fc1, dln2)
            release(dh)
            dy = G((rows, D))
            dy_sum = ln_bwd(bwd, dln2, sv["y"], sv["mu2"], sv["rs2"], b.ln2, dz, dy, rows, D, want_sum=True)
            release(dln2)
            release(dz)
            # ---- attention branch: y = out_proj(mha(in_proj(ln1(x)))) + x
            bias_grad(bwd, dy, rows, D, b.out.dbias, dy_sum)
            wgrad(bwd, sv["att"], (rows, 1, 1, D), dy, (rows, 1, 1, D), 1, 1, b.out.g)
            datt = G((rows, D))
            dgrad_lin(bwd, dy, rows, b.out, datt)
            dqkv = G((rows, 3 * D))
            bwd.append((lib.pfr_mha_bwd, (sv["qkv"].data_ptr(), sv["att"].data_ptr(), datt.data_ptr(), sv["lse"].data_ptr(),
                                          dqkv.data_ptr(), did, N, S, heads, hd, scale)))
            release(datt)
            colsum(bwd, dqkv, rows, 3 * D, b.qkv.dbias)
            wgrad(bwd, sv["ln1"], (rows, 1, 1, D), dqkv, (rows, 1, 1, 3 * D), 1, 1, b.qkv.g)
            dln1 = G((rows, D))
            dgrad_lin(bwd, dqkv, rows, b.qkv, dln1)
            release(dqkv)
            dx = G((rows, D))
            dz_sum = ln_bwd(bwd, dln1, sv["x"], sv["mu1"], sv["rs1"], b.ln1, dy, dx, rows, D, want_sum=True)
            release(dln1)
            release(dy)
            dz = dx
            if li and li % self.mark_every == 0:
                mark(bwd, b.off)
        # ---- token assembly: position-embedding and class-token gradients, dout[:, 1:] for the patch embedding
        dpatch = G((N, OH, OW, D))
        bwd.append((lib.pfr_vit_tokens_bwd, (dz.data_ptr(), dpatch.data_ptr(), self.dpos.data_ptr(), self.dcls.data_ptr(), did, N, S, D)))
        release(dz)
        colsum(bwd, dpatch, N * OH * OW, D, cv.dbias)
        wgrad(bwd, x_nhwc, (N, H, W, self.cp), dpatch, (N, OH, OW, D), f, f, cv.g_conv)
        side(bwd, (SIDE, (lib.pfr_nhwc_to_nchw_f32, (cv.g_conv.data_ptr(), cv.g.data_ptr(), cv.out, cv.cin, f * f, cv.cinp, 0))))
        mark(bwd, 0, last=True)
        plan.meta["n_side"] = nside[0]
        if self.ws is None or self.ws.numel() < ws_need[0]:
            self.ws = torch.empty(ws_need[0], dtype=torch.float32, device=dev)
        plan.ops = fwd + bwd
        return plan

    def forward(self, x, train, with_backward, ticket=None):
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise PfrError(f"expected NCHW input with {self.in_channels} channels, got {tuple(x.shape)}")
        if x.shape[2] != self.image_size or x.shape[3] != self.image_size:
            raise ValueError(f"ViT: the position embedding was built for {self.image_size}x{self.image_size} images, got "
                             f"{x.shape[2]}x{x.shape[3]} (no position interpolation)")
        if train and self._p_drop > 0:
            raise PfrError("HIP ViT path: Dropout with p > 0 does not run on the device in training mode; build the model with "
                           "dropout=0 and attention_dropout=0")
        x = x.float().contiguous()
        N, _, H, W = x.shape
        plan = self.acquire_plan(N, H, W, with_backward, ticket=ticket if with_backward else None)
        if with_backward:
            self._fresh(plan)
        stream = torch.cuda.current_stream().cuda_stream
        self.refresh_weights(stream, for_backward=with_backward)
        lib.pfr_nchw_to_nhwc(x.data_ptr(), plan.meta["x_nhwc"].data_ptr(), self.did, N, x.shape[1], H, W, self.cp, stream)
        self._run_fwd(plan, stream)
        self._last_plan = plan
        return plan.meta["emb"]

    def backward(self, demb, plan=None):
        plan = plan if plan is not None else self._last_plan
        self._begin_backward(plan, demb)
        # As in SwinEngine: the plan's gradient launches overwrite their slices; a second backward before zero_grad sets the previous
        # sum aside and adds it back
        prev = self.grad.clone() if self.first_param.grad is not None else None
        hook = self.grad_ready_hook
        if prev is not None or any(self._plan_busy(q) for q in self.plans.values()):
            hook = None
        self._run_bwd(plan, "bwd", hook, hook)
        if prev is not None:
            self.grad.add_(prev)
        self.attach_grads()


vit_forward = engine_forward
