"""The convolution oracle of the exact GPU tests (tests/conv_oracle.py), checked without a GPU: (a) the float64 references written as the
definition equal float64 F.conv2d / autograd on every geometry of tests/test_conv_exact_gpu.py; (b) the integer data keeps every expected
value exactly representable in the output format (an arithmetic guarantee of the generators, asserted on the data all the same);
(c) the references are not trivially sparse, in general and in each edge region; (d) the comparison the GPU tests assert with detects a
deliberately broken copy of the reference."""
import pytest
import torch
import torch.nn.functional as F

import conv_oracle as O

F64 = torch.float64
ALL_FWD = O.FWD_GEOMS + O.EPI_GEOMS + O.SCONV_GEOMS + O.SCONV3_GEOMS + O.SLIN_GEOMS
nchw = lambda t: t.permute(0, 3, 1, 2)
nhwc = lambda t: t.permute(0, 2, 3, 1)


def _conv2d(x, w, stride, pad, ohw=None):
    """float64 F.conv2d on the library's layouts; ohw: the window of the space-to-depth stem (extra zero border behind, output cut)"""
    if ohw is not None:
        R = w.shape[1]
        xb = F.pad(nchw(x), (pad, R, pad, R))
        return nhwc(F.conv2d(xb, nchw(w), stride=stride))[:, :ohw[0], :ohw[1]]
    return nhwc(F.conv2d(nchw(x), nchw(w), stride=stride, padding=pad))


@pytest.mark.parametrize("geom", sorted(set(ALL_FWD)) + [O.STEM_GEOM])
def test_forward_reference_equals_conv2d_and_is_exactly_representable(geom):
    stem = geom == O.STEM_GEOM
    N, H, W, C, Cout, R, stride, pad = geom
    epis = [""] + (O.EPIS if geom in O.EPI_GEOMS else []) + (["bias", "bias+res"] if geom in O.SLIN_GEOMS else []) + \
        (["bias+relu"] if stem else []) + (["join"] if geom in O.SCONV_JOIN_GEOMS else [])
    for epi in epis:
        c = O.fwd_case(geom, epi, (H, W) if stem else None, 12 if stem else None)
        for kp in ((8, 4) if "join" in c["flags"] and Cout % 8 == 0 else (8,)):
            ref = O.fwd_ref(c, kp)
            want = _conv2d(O.apply_prologue(c["x"], c["pro"]), c["w"], stride, pad, c["ohw"] if stem else None)
            if c["bias"] is not None:
                want = want + c["bias"]
            if c["res"] is not None:
                want = want + c["res"] * (O.mask_bits(c["mask%d" % kp], kp).reshape(want.shape) if "join" in c["flags"] else 1)
            if c["acc"] is not None:
                want = want + c["acc"]
            if c["relu"]:
                want = F.relu(want)
            assert torch.equal(ref, want), (geom, epi)                                     # (a): integers, so equal and not merely close
            assert ref.abs().max().item() <= 256 and torch.equal(ref, ref.round())        # (b): exact in bf16 (and in fp32)
            assert torch.equal(ref.bfloat16().to(F64), ref)
            assert c["x"].abs().max() <= 2 and int((c["w"] != 0).reshape(Cout, -1).sum(1).max()) <= (O.PRO_NNZ if c["pro"] else O.NNZ)
            # (c) an output ReLU alone zeroes the negative half of a symmetric distribution: a third must remain there
            assert (ref != 0).double().mean().item() >= (1 / 3 if c["relu"] else 0.5), (geom, epi)
            for name, region in O.edge_regions(ref).items():
                assert bool((region != 0).any()), (geom, epi, name)


@pytest.mark.parametrize("geom", O.DGRAD_GEOMS + O.SCONV3_GEOMS)
@pytest.mark.parametrize("accumulate", [False, True])
def test_data_gradient_reference_equals_autograd(geom, accumulate):
    N, H, W, C, Cout, R, stride, pad = geom
    c = O.dgrad_case(geom, accumulate)
    x = torch.zeros(N, C, H, W, dtype=F64, requires_grad=True)
    F.conv2d(x, nchw(c["w"]), stride=stride, padding=pad).backward(nchw(c["dy"]))
    want = nhwc(x.grad) + (c["acc"] if accumulate else 0)
    assert torch.equal(c["ref"], want)
    assert c["ref"].abs().max().item() <= 256 and torch.equal(c["ref"].bfloat16().to(F64), c["ref"])
    assert int((c["w"] != 0).permute(3, 0, 1, 2).reshape(C, -1).sum(1).max()) <= O.NNZ
    if R == 1 and stride == 2 and not accumulate:          # only parity class (0, 0) has taps: exact zeros elsewhere
        assert not bool(c["ref"][:, 1::2].any()) and not bool(c["ref"][:, :, 1::2].any())
        assert (c["ref"][:, ::2, ::2] != 0).double().mean().item() >= 0.5
    else:
        assert (c["ref"] != 0).double().mean().item() >= 0.5
        for name, region in O.edge_regions(c["ref"]).items():
            assert bool((region != 0).any()), (geom, name)


WG = sorted(set(O.WGRAD_GEOMS + [O.WGRAD_BIG_GEOM, O.SWGRAD_GEOM] + O.WGRAD9_GEOMS))


@pytest.mark.parametrize("geom", WG)
def test_weight_gradient_reference_equals_autograd(geom):
    N, H, W, C, Cout, R, stride, pad = geom
    for pro in ["", "pro", "prorelu"] if geom in O.WGRAD_PRO_GEOMS else [""]:
        for scale, accumulate in ((1.0, False), (0.5, True), (4.0, True)):
            c = O.wgrad_case(geom, pro, accumulate)
            ref = O.conv_wgrad_ref(c["x"], c["dy"], R, R, stride, pad, c["pro"], scale, c["acc"])
            w = torch.zeros(Cout, C, R, R, dtype=F64, requires_grad=True)
            F.conv2d(nchw(O.apply_prologue(c["x"], c["pro"])), w, stride=stride, padding=pad).backward(nchw(c["dy"]))
            want = nhwc(w.grad) * scale + (c["acc"] if accumulate else 0)
            assert torch.equal(ref, want), (geom, pro, scale)
            assert ref.abs().max().item() < 2 ** 24 and torch.equal(ref.float().to(F64), ref)      # (b) fp32 output
            if N * c["dy"].shape[1] * c["dy"].shape[2] > 1:
                assert (ref != 0).double().mean().item() >= 0.5, (geom, pro, scale)


def test_comparison_detects_a_broken_reference():
    """(d) one tap dropped at one border pixel, one channel shifted, one tail row left unwritten: each must fail the exact comparison,
    and the same defects in a real-valued case must fail the per-element bound"""
    geom = O.FWD_GEOMS[0]
    c = O.fwd_case(geom)
    ref = O.fwd_ref(c)
    O.assert_exact(ref.bfloat16(), ref)
    O.assert_exact(ref.float(), ref)
    dropped = O.fwd_ref(c, drop_tap=(0, 1, 0, 4))          # tap (0, 1) reads the zero border above pixel (0, 4): "pad test dropped"
    assert torch.equal(dropped, ref)                       # ... so leaving it out changes nothing; the defect is READING something there
    dropped = O.fwd_ref(c, drop_tap=(1, 1, 0, 4))
    assert not torch.equal(dropped, ref)
    shifted = ref.clone()
    shifted[..., 70] = ref[..., 71]
    unwritten = ref.clone()
    unwritten.reshape(-1, 72)[161] = float("nan")
    for broken in (dropped, shifted, unwritten):
        for dt in (torch.bfloat16, torch.float32):
            with pytest.raises(AssertionError):
                O.assert_exact(broken.to(dt), ref)
    # the per-element bound: real-valued data, one rounding to bf16 of the exact value passes, the broken copies do not
    g = O.rng(5)
    x = torch.randn(2, 9, 9, 64, generator=g).bfloat16().to(F64)
    w = (torch.randn(72, 3, 3, 64, generator=g) / 24).bfloat16().to(F64)
    r = O.conv_fwd_ref(x, w, 1, 1)
    bound = O.rounding_bound([r], 576, O.conv_fwd_ref(x.abs(), w.abs(), 1, 1), True)
    O.assert_within(r.bfloat16(), r, bound)
    with pytest.raises(AssertionError):
        O.assert_within(O.conv_fwd_ref(x, w, 1, 1, drop_tap=(1, 1, 0, 4)).bfloat16(), r, bound)
    s = r.clone()
    s[..., 70] = r[..., 71]
    with pytest.raises(AssertionError):
        O.assert_within(s.bfloat16(), r, bound)
    with pytest.raises(AssertionError):
        O.assert_within(torch.full_like(r, float("nan")), r, bound)


def test_seeds_are_fixed_per_case():
    a = O.fwd_case.__wrapped__(O.FWD_GEOMS[1], "bias")
    b = O.fwd_case(O.FWD_GEOMS[1], "bias")
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["w"], b["w"]) and torch.equal(a["bias"], b["bias"])
