"""ViTEngine — executes the Vision Transformer feature extractor (forward, backward) on the gfx950 kernels.

Same design as models/_swin_engine.SwinEngine: flat fp32 master / gradient buffers (the module's nn.Parameters become views,
torchvision's state-dict names unchanged), compute-dtype shadow, one pre-built plan of C-ABI calls per input shape; the plan runtime
and the PlanBuilder that build_plan emits through are models/_plan_engine.py, the Linear / LayerNorm emitters models/_plan_layers.py.
Tokens are [B, S, D] rows end to end.

Mapping (models/vit.py):
  conv_proj (patch x patch, stride patch)          → pfr_conv2d_fwd on NHWC (weights re-laid out per step), pfr_conv2d_wgrad; no data gradient
  [class_token; patches] + pos_embedding           → pfr_vit_tokens_fwd / pfr_vit_tokens_bwd (csrc/pfr_mha.hip)
  LayerNorm                                        → pfr_layernorm_fwd / pfr_layernorm_bwd_dxsum
  in_proj / out_proj / mlp.3 / heads               → pfr_conv2d_fwd (GEMM, bias and residual-add fused in the epilogue), pfr_conv2d_wgrad
  mlp.0 + GELU                                     → pfr_gemm_act (GELU in the epilogue; its backward in the data-gradient GEMM's)
  attention over the whole sequence                → pfr_mha_fwd / pfr_mha_bwd (csrc/pfr_mha.hip)
  encoder.ln on the class-token rows, heads        → pfr_vit_cls_fwd / pfr_vit_cls_bwd, pfr_layernorm_*, pfr_conv2d_fwd
"""
import torch
import torch.nn as nn

from .._hip import lib, PfrError
from .._hip.cplan import SIDE
from ._plan_engine import PlanEngine, PlanBuilder, Plan, engine_forward
from ._plan_layers import gemm, dgrad_lin, ln_fwd, ln_bwd, bias_grad


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
        offs = self._adopt_flat(named)

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
        pb = PlanBuilder(plan, T, dev, did, self.pool_depth)
        A, fwd, bwd = pb.A, pb.fwd, pb.bwd

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
            ln1, mu1, rs1 = ln_fwd(pb, x, b.ln1, rows, D)
            qkv = A((rows, 3 * D))
            gemm(pb, ln1, rows, D, b.qkv, qkv)
            att = A((rows, D))
            lse = A((N, heads, S), torch.float32)
            fwd.append((lib.pfr_mha_fwd, (qkv.data_ptr(), att.data_ptr(), lse.data_ptr(), did, N, S, heads, hd, scale)))
            y = A((rows, D))
            gemm(pb, att, rows, D, b.out, y, residual=x)
            ln2, mu2, rs2 = ln_fwd(pb, y, b.ln2, rows, D)
            h1 = A((rows, Hd))
            h2 = A((rows, Hd))
            # GELU in the fc1 GEMM's epilogue (writes the pre-activation h1 and h2 = gelu(h1))
            fwd.append((lib.pfr_gemm_act, (ln2.data_ptr(), b.fc1.w.data_ptr(), h2.data_ptr(), did, rows, D, Hd, b.fc1.bias.data_ptr(), 2,
                                           h1.data_ptr())))
            z = A((rows, D))
            gemm(pb, h2, rows, Hd, b.fc2, z, residual=y)
            saved.append(dict(x=x, ln1=ln1, mu1=mu1, rs1=rs1, qkv=qkv, att=att, lse=lse, y=y, ln2=ln2, mu2=mu2, rs2=rs2, h1=h1, h2=h2))
            x = z
        # encoder.ln on the class-token rows only (row 0 of every sample is all the head reads)
        ctok = A((N, D))
        fwd.append((lib.pfr_vit_cls_fwd, (x.data_ptr(), ctok.data_ptr(), did, N, S, D)))
        hln, hmu, hrs = ln_fwd(pb, ctok, self.head_ln, N, D)
        emb = A((N, self.emb_dim), torch.float32)
        gemm(pb, hln, N, D, self.head_fc, emb)
        plan.ops = fwd
        plan.meta.update(x_nhwc=x_nhwc, emb=emb, n_fwd=len(fwd))
        if not with_backward:
            return plan

        # ================================================================= backward (stream roles, buffer pool: PlanBuilder)
        G, release, side, wgrad, colsum, pend_cs, mark = pb.G, pb.release, pb.side, pb.wgrad, pb.colsum, pb.pend_cs, pb.mark

        # ---- heads, encoder.ln on the class-token rows
        demb = A((N, self.emb_dim))
        plan.meta["demb"] = demb
        hf = self.head_fc
        colsum(demb, N, hf.out, hf.dbias)
        wgrad(hln, (N, 1, 1, D), demb, (N, 1, 1, hf.out), 1, 1, 0, hf.g)
        dhln = G((N, D))
        dgrad_lin(pb, demb, N, hf, dhln)
        dctok = G((N, D))
        ln_bwd(pb, dhln, ctok, hmu, hrs, self.head_ln, None, dctok, N, D)
        release(dhln)
        dz = G((rows, D))
        bwd.append((lib.pfr_vit_cls_bwd, (dctok.data_ptr(), dz.data_ptr(), did, N, S, D)))
        release(dctok)
        dz_sum = None   # column sums of dz left by the pass that produced it
        mark(self.head_off)
        for li in range(len(self.layers) - 1, -1, -1):
            b, sv = self.layers[li], saved[li]
            Hd = b.fc1.out
            # ---- MLP branch: z = fc2(gelu(fc1(ln2(y)))) + y
            bias_grad(pb, dz, rows, D, b.fc2.dbias, dz_sum)
            wgrad(sv["h2"], (rows, 1, 1, Hd), dz, (rows, 1, 1, D), 1, 1, 0, b.fc2.g)
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
            wgrad(sv["ln2"], (rows, 1, 1, D), dh, (rows, 1, 1, Hd), 1, 1, 0, b.fc1.g)
            dln2 = G((rows, D))
            dgrad_lin(pb, dh, rows, b.fc1, dln2)
            release(dh)
            dy = G((rows, D))
            dy_sum = ln_bwd(pb, dln2, sv["y"], sv["mu2"], sv["rs2"], b.ln2, dz, dy, rows, D, want_sum=True)
            release(dln2)
            release(dz)
            # ---- attention branch: y = out_proj(mha(in_proj(ln1(x)))) + x
            bias_grad(pb, dy, rows, D, b.out.dbias, dy_sum)
            wgrad(sv["att"], (rows, 1, 1, D), dy, (rows, 1, 1, D), 1, 1, 0, b.out.g)
            datt = G((rows, D))
            dgrad_lin(pb, dy, rows, b.out, datt)
            dqkv = G((rows, 3 * D))
            bwd.append((lib.pfr_mha_bwd, (sv["qkv"].data_ptr(), sv["att"].data_ptr(), datt.data_ptr(), sv["lse"].data_ptr(),
                                          dqkv.data_ptr(), did, N, S, heads, hd, scale)))
            release(datt)
            colsum(dqkv, rows, 3 * D, b.qkv.dbias)
            wgrad(sv["ln1"], (rows, 1, 1, D), dqkv, (rows, 1, 1, 3 * D), 1, 1, 0, b.qkv.g)
            dln1 = G((rows, D))
            dgrad_lin(pb, dqkv, rows, b.qkv, dln1)
            release(dqkv)
            dx = G((rows, D))
            dz_sum = ln_bwd(pb, dln1, sv["x"], sv["mu1"], sv["rs1"], b.ln1, dy, dx, rows, D, want_sum=True)
            release(dln1)
            release(dy)
            dz = dx
            if li and li % self.mark_every == 0:
                mark(b.off)
        # ---- token assembly: position-embedding and class-token gradients, dout[:, 1:] for the patch embedding
        dpatch = G((N, OH, OW, D))
        bwd.append((lib.pfr_vit_tokens_bwd, (dz.data_ptr(), dpatch.data_ptr(), self.dpos.data_ptr(), self.dcls.data_ptr(), did, N, S, D)))
        release(dz)
        colsum(dpatch, N * OH * OW, D, cv.dbias)
        wgrad(x_nhwc, (N, H, W, self.cp), dpatch, (N, OH, OW, D), f, f, 0, cv.g_conv)
        side((SIDE, (lib.pfr_nhwc_to_nchw_f32, (cv.g_conv.data_ptr(), cv.g.data_ptr(), cv.out, cv.cin, f * f, cv.cinp, 0))))
        mark(0, last=True)
        return pb.finish(self)

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
        return self._forward_plan(x, N, H, W, with_backward, with_backward=with_backward, ticket=ticket)


vit_forward = engine_forward
