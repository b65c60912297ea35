"""csrc/pfr_swin.hip window attention through the C-ABI against a DENSE fp64 reference on the CPU: pfr_window_bias_table,
pfr_window_attn_fwd / pfr_window_attn_bwd in their three kernel families: fp32 register-blocked, bf16 register-blocked (the `attn_mfma`
knob at 0, or any head_dim != 32) and bf16 one-wave MFMA (head_dim 32).

The reference does not partition into windows: it is masked attention over all H·W tokens of an image, the mask and the bias index
taken from each token's rolled coordinates (_token_geometry).  test_dense_reference_matches_the_model_core pins it on the CPU to the
core of models/swin.py::WindowAttention.forward (1e-12 absolute) for shift in {0, w//2}, and to the same core with _shift_mask
restated at d = shift for the other shifts.  The reference is fed the inputs AS ROUNDED to the kernel's dtype (and the fp32-rounded
scale), so what is measured is the kernel's own error.

Geometries: non-square grids (nwh != nww), grids of 1 / 6 / 9 / 30 / 36 workgroups (the `n < 8` and `rem != 0` branches of the XCD
remap), w = 8 (64 tokens, no padding rows, 225 table entries), w = 2 .. 5 (the second MFMA query half is padding only), head dims
4 .. 28, every shift in {0, 1, w//2, w-1}.  Every run has 4096 sentinel elements behind `out`, `dqkv` and `dpos_part` and NaN in
front of them, so a window-head that is skipped, or a store behind a buffer, fails the run that made it.

Bounds: those of tests/test_mha_gpu.py and tests/test_swin_gpu.py::test_window_attention_kernel (relative L2: 2e-5 fp32, 2e-2 bf16).
Measured on an MI355X over all cases of test_window_attention_vs_fp64 (relative L2, smallest .. largest):
  fp32 register-blocked (52 cases): out 5e-8 .. 2.5e-7, dqkv 6e-8 .. 2.6e-7 (dq, dk, dv each <= 2.9e-7), dpos 1.0e-7 .. 3.8e-7
  bf16 register-blocked (41 cases): out 1.5e-3 .. 1.8e-3, dqkv 1.6e-3 .. 1.8e-3 (dq, dk, dv each <= 1.9e-3), dpos 9e-8 .. 2.3e-7
  bf16 MFMA (29 cases):             out 1.5e-3 .. 1.8e-3, dqkv 2.0e-3 .. 2.4e-3 (dq <= 2.6e-3, dk <= 2.8e-3, dv <= 2.4e-3), dpos 1.0e-7 .. 2.5e-7
With one query row times 60 (scaled scores up to 294): fp32 dk 2.4e-6, everything else as above; that row's out 4.7e-7 fp32, 1.0e-3 bf16.
No case uses more than 15 % of its bound.  (dpos is accumulated in fp32 in every family, hence its fp32-sized error in bf16.)
Two runs give the same bits in out and dqkv on every family and in the MFMA kernel's dpos_part; the register-blocked backward's
dpos_part differs in its last bits from run to run (atomicAdd on LDS floats)."""
import ctypes
import functools
import math

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda"
SENT = 4096
KNOB = b"attn_mfma"
FAMILIES = {"fp32": torch.float32, "bf16_rb": torch.bfloat16, "bf16_mfma": torch.bfloat16}
TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2}

# (B, H, W, heads, hd, w)
GEOMS_HD32 = [(2, 14, 21, 3, 32, 7), (1, 7, 7, 1, 32, 7), (1, 7, 21, 3, 32, 7), (1, 16, 8, 3, 32, 8), (1, 10, 15, 5, 32, 5),
              (3, 8, 12, 2, 32, 4), (2, 4, 6, 1, 32, 2), (1, 6, 9, 2, 32, 3)]
GEOMS_HD8 = [(2, 14, 7, 2, 16, 7), (1, 8, 8, 3, 24, 8), (2, 8, 4, 1, 8, 4)]          # register-blocked kernels in both dtypes
GEOMS_HD4 = [(1, 6, 3, 1, 4, 3), (1, 14, 14, 2, 12, 7), (1, 5, 10, 1, 28, 5)]         # fp32 only: hd a multiple of 4, not of 8
HOST_GEOMS = [(2, 14, 21, 3, 32, 7), (1, 8, 8, 1, 32, 8), (1, 7, 7, 2, 16, 7), (3, 8, 12, 2, 8, 4), (1, 10, 15, 5, 32, 5),
              (2, 6, 3, 1, 4, 3), (1, 16, 8, 3, 32, 8)]


def _shifts(w):
    return sorted({s for s in (0, 1, w // 2, w - 1) if s < w})


def _cases():
    out = []
    for fam, geoms in (("fp32", GEOMS_HD32 + GEOMS_HD8 + GEOMS_HD4), ("bf16_rb", GEOMS_HD32 + GEOMS_HD8), ("bf16_mfma", GEOMS_HD32)):
        for g in geoms:
            for s in _shifts(g[5]):
                out.append(pytest.param(fam, g, s, id=f"{fam}-{'x'.join(map(str, g))}-s{s}"))
    return out


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ------------------------------------------------------------------------------------------------ the fp64 reference
def _token_geometry(H, W, w, shift):
    """per token (y, x) of an image, flattened: the group (window and the two wrap flags, from the ROLLED coordinates) inside which it
    attends, and its position (iy, ix) inside the window"""
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    yr, xr = (y - shift) % H, (x - shift) % W
    fy, fx = (yr >= H - shift).long(), (xr >= W - shift).long()            # both all false at shift = 0
    group = (((yr // w) * (W // w) + xr // w) * 2 + fy) * 2 + fx
    return group.flatten(), (yr % w).flatten(), (xr % w).flatten()


def _reference(qkv, pos, dout, heads, w, shift, scale):
    """dense masked attention in fp64: out [B,H,W,C], dqkv [B,H,W,3C], dpos [2w-1,2w-1]"""
    B, H, W, C3 = qkv.shape
    C, N = C3 // 3, H * W
    hd = C // heads
    x = qkv.double().requires_grad_(True)
    p = pos.double().requires_grad_(True)
    q, k, v = (t.reshape(B, N, heads, hd).permute(0, 2, 1, 3) for t in x.reshape(B, N, C3).split(C, dim=-1))
    group, iy, ix = _token_geometry(H, W, w, shift)
    bias = p[iy[None, :] - iy[:, None] + w - 1, ix[None, :] - ix[:, None] + w - 1]           # [i][j]
    s = q @ k.transpose(-1, -2) * scale + bias
    s = s.masked_fill(group[:, None] != group[None, :], float("-inf"))
    out = (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, H, W, C)
    out.backward(dout.double())
    return out.detach(), x.grad, p.grad


def _shift_mask(w, d, vertical):
    """models/swin.py::_shift_mask restated for any displacement d"""
    idx = torch.arange(w * w)
    part = ((idx // w) if vertical else (idx % w)) >= (w - d)
    m = torch.zeros(w * w, w * w, dtype=torch.float64)
    m[part[:, None] != part[None, :]] = float("-inf")
    return m


def _model_core(qkv, pos, dout, heads, w, shift):
    """fp64: everything of WindowAttention.forward between to_qkv and to_out, with the model's own window partition, relative
    indices and (at shift = w//2, the only shift the model knows) its own masks"""
    import pets_face_recognition_amd.models.swin as S
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    att = S.WindowAttention(C, heads, C // heads, shift > 0 and shift == w // 2, w, True)
    x0 = qkv.double().requires_grad_(True)
    p = pos.double().requires_grad_(True)
    x = torch.roll(x0, (-shift, -shift), (1, 2)) if shift else x0
    gh, gw = H // w, W // w
    q, k, v = (att._windows(t, B, gh, gw) for t in x.chunk(3, dim=-1))
    dots = torch.matmul(q, k.transpose(-1, -2)) * att.scale
    ri = att.relative_indices
    dots = dots + p[ri[:, :, 0], ri[:, :, 1]]
    if shift:
        ul, lr = _shift_mask(w, shift, True), _shift_mask(w, shift, False)
        if att.shifted:
            assert torch.equal(ul, att.upper_lower_mask.double()) and torch.equal(lr, att.left_right_mask.double())
        dots[:, :, -gw:] += ul
        dots[:, :, gw - 1::gw] += lr
    out = torch.matmul(dots.softmax(dim=-1), v)
    out = out.view(B, heads, gh, gw, w, w, -1).permute(0, 2, 4, 3, 5, 1, 6).reshape(B, H, W, -1)
    if shift:
        out = torch.roll(out, (shift, shift), (1, 2))
    out.backward(dout.double())
    return out.detach(), x0.grad, p.grad, att.scale


def _inputs(geom, dtype, seed=0, big_row=None):
    """qkv [B,H,W,3C] with q, k ~ N(0, 2): the scaled scores q·k/sqrt(hd) have a standard deviation of about 2 (neither uniform nor
    one-hot); v, dout, pos ~ N(0, 1); all rounded to `dtype`.  big_row = (b, y, x, factor) multiplies one token's query rows."""
    B, H, W, heads, hd, w = geom
    g = torch.Generator().manual_seed(100000 * H + 1000 * W + 100 * heads + 10 * w + hd + B + 7919 * seed)
    C = heads * hd
    qkv = torch.randn(B, H, W, 3 * C, generator=g)
    qkv[..., :2 * C] *= math.sqrt(2.0)
    if big_row is not None:
        b, y, x, f = big_row
        qkv[b, y, x, :C] *= f
    dout = torch.randn(B, H, W, C, generator=g)
    pos = torch.randn(2 * w - 1, 2 * w - 1, generator=g)
    return qkv.to(dtype).float(), pos.to(dtype).float(), dout.to(dtype).float()


def _scale(hd):
    return torch.tensor(hd ** -0.5, dtype=torch.float32).item()          # what the kernel receives


@functools.lru_cache(maxsize=None)
def _case(geom, shift, dtype):
    """inputs and their fp64 results, computed once per (geometry, shift, dtype) and shared by the tests (nobody writes to them)"""
    qkv, pos, dout = _inputs(geom, dtype)
    return (qkv, pos, dout) + _reference(qkv, pos, dout, geom[3], geom[5], shift, _scale(geom[4]))


def test_dense_reference_matches_the_model_core():
    """CPU, fp64: the dense reference against the windowed core of the model, forward, dqkv and dpos, 1e-12 absolute"""
    worst = 0.0
    for geom in HOST_GEOMS:
        B, H, W, heads, hd, w = geom
        for shift in _shifts(w):
            qkv, pos, dout = _inputs(geom, torch.float32, seed=1)
            o_m, g_m, p_m, scale = _model_core(qkv, pos, dout, heads, w, shift)
            o_r, g_r, p_r = _reference(qkv, pos, dout, heads, w, shift, scale)
            e = [(a - b).abs().max().item() for a, b in ((o_r, o_m), (g_r, g_m), (p_r, p_m))]
            print(f"{geom} shift {shift}: out {e[0]:.1e} dqkv {e[1]:.1e} dpos {e[2]:.1e}")
            assert torch.isfinite(o_r).all() and torch.isfinite(g_r).all() and torch.isfinite(p_r).all()
            assert max(e) < 1e-12, (geom, shift, e)
            worst = max(worst, max(e))
    print(f"largest absolute difference {worst:.1e}")


# ------------------------------------------------------------------------------------------------ the kernels
def _knob():
    from pets_face_recognition_amd._hip import lib
    v = ctypes.c_int(-1)
    lib.pfr_get_tuning(KNOB, ctypes.byref(v))
    return v.value


@pytest.fixture(autouse=True)
def _knob_is_back_at_one(request):
    yield
    if request.node.get_closest_marker("gpu") is not None and torch.cuda.is_available():
        assert _knob() == 1


def _bias_table(pos, w, shift):
    """device table [8][64][64] from pfr_window_bias_table, NaN before the launch"""
    from pets_face_recognition_amd._hip import lib
    n = lib.pfr_window_bias_table_floats(w)
    assert n == 8 * 64 * 64
    tab = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    pd = pos.to(DEV, torch.float32).contiguous()
    lib.pfr_window_bias_table(pd.data_ptr(), tab.data_ptr(), w, shift, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return tab


def _guarded(n, dtype):
    """n elements of NaN (every one has to be written) and SENT sentinel elements behind them (none may be)"""
    t = torch.full((n + SENT,), float("nan"), dtype=dtype, device=DEV)
    t[n:] = -7.0
    return t


def _run(qkv, pos, dout, geom, shift, family, finite=True):
    """forward and backward on the device -> out [B,H,W,C], dqkv [B,H,W,3C], dpos_part [nblk][(2w-1)²].  bf16_rb at hd = 32 needs the
    knob at 0 (any other head_dim takes the register-blocked kernels by itself); the knob is back at 1 whatever happens.  Checked on
    every call: the sentinels are untouched and (unless the inputs carry NaN on purpose) every element in front of them is finite."""
    from pets_face_recognition_amd._hip import lib, dtype_id
    B, H, W, heads, hd, w = geom
    dtype = FAMILIES[family]
    if family == "bf16_mfma":
        assert hd == 32 and w * w <= 64
    C = heads * hd
    nblk, ntab = B * (H // w) * (W // w) * heads, (2 * w - 1) ** 2
    n_o, n_g, n_p = B * H * W * C, B * H * W * 3 * C, nblk * ntab
    st = torch.cuda.current_stream().cuda_stream
    did = dtype_id(dtype)
    tab = _bias_table(pos, w, shift)
    qd = qkv.to(DEV, dtype).contiguous()
    dd = dout.to(DEV, dtype).contiguous()
    ob, gb, pb = _guarded(n_o, dtype), _guarded(n_g, dtype), _guarded(n_p, torch.float32)
    try:
        lib.pfr_set_tuning(KNOB, 0 if (family == "bf16_rb" and hd == 32) else 1)
        lib.pfr_window_attn_fwd(qd.data_ptr(), tab.data_ptr(), ob.data_ptr(), did, B, H, W, heads, hd, w, shift, _scale(hd), st)
        lib.pfr_window_attn_bwd(qd.data_ptr(), tab.data_ptr(), dd.data_ptr(), gb.data_ptr(), pb.data_ptr(), did, B, H, W, heads, hd, w,
                                shift, _scale(hd), st)
        torch.cuda.synchronize()
    finally:
        lib.pfr_set_tuning(KNOB, 1)
    for t, n, name in ((ob, n_o, "out"), (gb, n_g, "dqkv"), (pb, n_p, "dpos_part")):
        assert torch.all(t[n:] == -7.0), f"store behind {name}"
        if finite:
            assert torch.isfinite(t[:n].float()).all(), f"{name}: an element was not written, or is not finite"
    return ob[:n_o].view(B, H, W, C).clone(), gb[:n_g].view(B, H, W, 3 * C).clone(), pb[:n_p].view(nblk, ntab).clone()


def _errors(res, ref, C):
    """relative L2 of out, dqkv, dq, dk, dv, dpos_part.sum(0) against the fp64 (out, dqkv, dpos)"""
    out, dqkv, dpart = res
    o_r, g_r, p_r = ref
    e = {"out": rel(out, o_r), "dqkv": rel(dqkv, g_r)}
    for i, n in enumerate(("dq", "dk", "dv")):
        e[n] = rel(dqkv[..., i * C:(i + 1) * C], g_r[..., i * C:(i + 1) * C])
    e["dpos"] = rel(dpart.double().sum(0), p_r.flatten())
    return e


def _fmt(e):
    return " ".join(f"{k} {v:.3e}" for k, v in e.items())


@gpu
@pytest.mark.parametrize("family,geom,shift", _cases())
def test_window_attention_vs_fp64(family, geom, shift):
    dtype = FAMILIES[family]
    qkv, pos, dout, *ref = _case(geom, shift, dtype)
    res = _run(qkv, pos, dout, geom, shift, family)
    e = _errors(res, ref, geom[3] * geom[4])
    print(f"{family} {geom} shift {shift}: {_fmt(e)}")
    assert max(e.values()) < TOL[dtype], e


def _token_rows(geom, shift, gy, gx):
    """[H*W] bool: the tokens of window (gy, gx), chosen in rolled coordinates"""
    B, H, W, heads, hd, w = geom
    group = _token_geometry(H, W, w, shift)[0]
    return (group >> 2) == gy * (W // w) + gx


@gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_window_isolation(family):
    """one whole window of image 0 (the last window row AND column: all four mask regions) is NaN in qkv and dout: every other
    window's out and dqkv, and the other window-heads' rows of dpos_part, are finite and bit-identical to the clean run (in the MFMA
    loader the padding rows read a valid row of the OWN window unconditionally and are zeroed by a select)"""
    geom, shift = (2, 14, 21, 3, 32, 7), 3
    B, H, W, heads, hd, w = geom
    qkv, pos, dout = _case(geom, shift, FAMILIES[family])[:3]
    clean = _run(qkv, pos, dout, geom, shift, family)
    gy, gx = H // w - 1, W // w - 1
    rows = _token_rows(geom, shift, gy, gx)
    assert rows.sum() == w * w
    bad = torch.zeros(B, H * W, dtype=torch.bool)
    bad[0] = rows
    bad = bad.view(B, H, W)
    q2, d2 = qkv.clone(), dout.clone()
    q2[bad] = float("nan")
    d2[bad] = float("nan")
    out, dqkv, dpart = _run(q2, pos, d2, geom, shift, family, finite=False)
    good = (~bad).to(DEV)
    for a, c in ((out, clean[0]), (dqkv, clean[1])):
        assert torch.isfinite(a[good].float()).all()
        assert torch.equal(a[good], c[good])
    unit0 = (gy * (W // w) + gx) * heads                       # image 0: dpos_part rows unit0 .. unit0 + heads - 1 are the NaN window's
    keep = torch.ones(dpart.shape[0], dtype=torch.bool, device=DEV)
    keep[unit0:unit0 + heads] = False
    assert torch.isfinite(dpart[keep]).all()
    if family == "bf16_mfma":
        assert torch.equal(dpart[keep], clean[2][keep])
    else:
        assert rel(dpart[keep], clean[2][keep]) < TOL[torch.float32]


@gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_head_isolation(family):
    """head 1's channels of every token are NaN in q, k, v and dout: heads 0 and 2 are finite and bit-identical to the clean run"""
    geom, shift = (2, 14, 21, 3, 32, 7), 3
    B, H, W, heads, hd, w = geom
    C = heads * hd
    qkv, pos, dout = _case(geom, shift, FAMILIES[family])[:3]
    clean = _run(qkv, pos, dout, geom, shift, family)
    q2, d2 = qkv.clone(), dout.clone()
    q2.view(B, H, W, 3, heads, hd)[..., 1, :] = float("nan")
    d2.view(B, H, W, heads, hd)[..., 1, :] = float("nan")
    out, dqkv, dpart = _run(q2, pos, d2, geom, shift, family, finite=False)
    for h in (0, 2):
        a, c = out.view(B, H, W, heads, hd)[..., h, :], clean[0].view(B, H, W, heads, hd)[..., h, :]
        assert torch.isfinite(a.float()).all() and torch.equal(a, c)
        a, c = dqkv.view(B, H, W, 3, heads, hd)[..., h, :], clean[1].view(B, H, W, 3, heads, hd)[..., h, :]
        assert torch.isfinite(a.float()).all() and torch.equal(a, c)
        assert torch.isfinite(dpart[h::heads]).all()


@gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_extreme_scores(family):
    """one token's query rows times 60: its scaled scores have a standard deviation of ~120; same bounds, also for that row alone"""
    geom, shift = (1, 14, 14, 2, 32, 7), 3
    B, H, W, heads, hd, w = geom
    dtype = FAMILIES[family]
    C = heads * hd
    y, x = 12, 11                                                # last window row and column, the 4 x 4 region in front of the wrap
    qkv, pos, dout = _inputs(geom, dtype, seed=3, big_row=(0, y, x, 60.0))
    group = _token_geometry(H, W, w, shift)[0]
    i = y * W + x
    allowed = group == group[i]
    s = (qkv[0, y, x, :hd].double() @ qkv[0].reshape(H * W, 3 * C)[allowed, C:C + hd].double().t()) * _scale(hd)
    assert s.abs().max() > 100                                   # the row really is extreme
    ref = _reference(qkv, pos, dout, heads, w, shift, _scale(hd))
    res = _run(qkv, pos, dout, geom, shift, family)
    e = _errors(res, ref, C)
    e["out[big row]"] = rel(res[0][0, y, x], ref[0][0, y, x])
    print(f"{family}: max |score| {s.abs().max():.0f}: {_fmt(e)}")
    assert max(e.values()) < TOL[dtype], e


@gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_two_runs_are_bit_identical(family):
    """out and dqkv on every family, dpos_part on the MFMA path (integer bins: order-independent).  The register-blocked backward
    accumulates its table with atomicAdd on LDS floats, whose order is not fixed: its dpos_part is compared at the fp32 bound."""
    geom, shift = (2, 14, 21, 3, 32, 7), 3
    qkv, pos, dout = _case(geom, shift, FAMILIES[family])[:3]
    a = _run(qkv, pos, dout, geom, shift, family)
    b = _run(qkv, pos, dout, geom, shift, family)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    print(f"{family}: dpos_part of two runs bit-identical: {torch.equal(a[2], b[2])}")
    if family == "bf16_mfma":
        assert torch.equal(a[2], b[2])
    else:
        assert rel(a[2], b[2]) < TOL[torch.float32]


@gpu
@pytest.mark.parametrize("geom", [(3, 8, 12, 2, 32, 4), (2, 14, 21, 3, 32, 7), (1, 16, 8, 3, 32, 8)], ids=["w4", "w7", "w8"])
def test_mfma_and_register_blocked_agree_with_fp64(geom):
    """bf16, hd = 32, the same inputs through both kernel pairs: each within the fp64 bounds.  Not bit-identical (the MFMA path rounds
    P to bf16 before P·V, the register-blocked one keeps it in fp32) — which also shows that the knob selects another kernel."""
    shift = geom[5] // 2
    qkv, pos, dout, *ref = _case(geom, shift, torch.bfloat16)
    res = {f: _run(qkv, pos, dout, geom, shift, f) for f in ("bf16_mfma", "bf16_rb")}
    for f, r in res.items():
        e = _errors(r, ref, geom[3] * geom[4])
        print(f"{f} {geom}: {_fmt(e)}")
        assert max(e.values()) < TOL[torch.bfloat16], (f, e)
    assert not (torch.equal(res["bf16_mfma"][0], res["bf16_rb"][0]) and torch.equal(res["bf16_mfma"][1], res["bf16_rb"][1]))


def _table_definition(pos, w, shift):
    """[4][64][64]: relative-position bias, −inf between the two sides of the wrap in the last window row (variant & 2) / column
    (variant & 1), −inf outside the w² x w² block"""
    nt = w * w
    i = torch.arange(nt)
    yi, xi = i // w, i % w
    bias = pos[yi[None, :] - yi[:, None] + w - 1, xi[None, :] - xi[:, None] + w - 1]
    py, px = yi >= w - shift, xi >= w - shift
    t = torch.full((4, 64, 64), float("-inf"))
    for var in range(4):
        b = bias.clone()
        if shift and var & 2:
            b[py[:, None] != py[None, :]] = float("-inf")
        if shift and var & 1:
            b[px[:, None] != px[None, :]] = float("-inf")
        t[var, :nt, :nt] = b
    return t


def _perm_index():
    """wa_perm_index restated: [var][it][jt][g][half][query][4] with i = 32 it + query, j = 32 jt + 8 g + 4 half + e"""
    var, i, j = torch.meshgrid(torch.arange(4), torch.arange(64), torch.arange(64), indexing="ij")
    it, il, jt, jl = i // 32, i % 32, j // 32, j % 32
    return ((((((var * 2 + it) * 2 + jt) * 4 + jl // 8) * 2 + (jl // 4) % 2) * 32 + il) * 4 + jl % 4).flatten()


@gpu
def test_bias_table_by_definition():
    idx = _perm_index()
    assert torch.equal(idx.sort().values, torch.arange(4 * 64 * 64))           # the access order is a permutation
    for w in (2, 3, 4, 5, 7, 8):
        pos = torch.randn(2 * w - 1, 2 * w - 1, generator=torch.Generator().manual_seed(w))
        for shift in _shifts(w):
            tab = _bias_table(pos, w, shift).cpu()
            assert not torch.isnan(tab).any(), "an entry of the table was not written"
            want = _table_definition(pos, w, shift).flatten()
            perm = torch.empty_like(want)
            perm[idx] = want
            assert torch.equal(tab[:4 * 64 * 64].view(torch.int32), want.view(torch.int32)), (w, shift)
            assert torch.equal(tab[4 * 64 * 64:].view(torch.int32), perm.view(torch.int32)), (w, shift)


@gpu
def test_refused_shapes_launch_nothing():
    from pets_face_recognition_amd._hip import lib, dtype_id, PfrError
    st = torch.cuda.current_stream().cuda_stream
    base = dict(B=1, H=14, W=14, heads=2, hd=32, w=7, shift=3, qkv=True)
    bad = [dict(w=9, H=18, W=18), dict(hd=40), dict(H=15), dict(W=15), dict(shift=7), dict(shift=-1), dict(qkv=False)]
    per_dtype = {torch.float32: [dict(hd=6)], torch.bfloat16: [dict(hd=12)]}
    tab = _bias_table(torch.zeros(13, 13), 7, 3)
    for dtype in (torch.float32, torch.bfloat16):
        did = dtype_id(dtype)
        n = 1 << 20                                          # far more than any of these shapes would touch
        qd = torch.zeros(n, dtype=dtype, device=DEV)
        out = torch.full((n,), -7.0, dtype=dtype, device=DEV)
        dqkv = torch.full((n,), -7.0, dtype=dtype, device=DEV)
        dpart = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
        for change in bad + per_dtype[dtype]:
            c = dict(base, **change)
            qp = qd.data_ptr() if c["qkv"] else 0
            geo = (c["B"], c["H"], c["W"], c["heads"], c["hd"], c["w"], c["shift"], c["hd"] ** -0.5, st)
            with pytest.raises(PfrError):
                lib.pfr_window_attn_fwd(qp, tab.data_ptr(), out.data_ptr(), did, *geo)
            with pytest.raises(PfrError):
                lib.pfr_window_attn_bwd(qp, tab.data_ptr(), qd.data_ptr(), dqkv.data_ptr(), dpart.data_ptr(), did, *geo)
        torch.cuda.synchronize()
        assert torch.all(out == -7.0) and torch.all(dqkv == -7.0) and torch.all(dpart == -7.0)


@gpu
def test_knob_is_restored_after_a_failing_run():
    """a run on the register-blocked bf16 kernels that raises inside (a refused shift) leaves the knob at 1"""
    from pets_face_recognition_amd._hip import PfrError
    geom = (1, 7, 7, 1, 32, 7)
    qkv, pos, dout = _case(geom, 0, torch.bfloat16)[:3]
    assert _knob() == 1
    with pytest.raises(PfrError):
        _run(qkv, pos, dout, geom, 7, "bf16_rb")
    assert _knob() == 1
