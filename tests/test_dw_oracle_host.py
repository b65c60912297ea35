"""The depthwise oracle of the exact GPU tests (tests/dw_oracle.py), checked without a GPU: (a) the float64 references written as the
definition equal float64 F.conv2d(groups=C) and its autograd; (b) every integer case tests/test_dw_exact_gpu.py runs keeps its range
assertions (they sit in the builders: building a case IS the check) and is not trivially sparse, in general and in each edge region;
(c) the comparison the GPU tests assert with sees one tap dropped at one pixel, and names the region it is in."""
import pytest
import torch
import torch.nn.functional as F

import dw_oracle as D
import test_dw_exact_gpu as G

F64 = torch.float64
nchw = lambda t: t.permute(0, 3, 1, 2)
nhwc = lambda t: t.permute(0, 2, 3, 1)
PLANES = [(2, 9, 7, 5), (1, 8, 10, 6), (2, 2, 3, 4)]          # odd, even, smaller than every K


def close(a, b):
    return (a - b).abs().max().item() <= 1e-12 * b.abs().max().item()


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["plain", "clamp", "silu"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("shape", PLANES, ids=lambda s: "x".join(map(str, s)))
def test_references_equal_conv2d_and_autograd(shape, K, stride, mode):
    N, H, W, C = shape
    g = D.rng(D._seed("host", shape, K, stride, mode))
    x = torch.randn(shape, generator=g, dtype=F64) * 3
    w = torch.randn(C, K, K, generator=g, dtype=F64)
    bias = torch.randn(C, generator=g, dtype=F64)
    act = (mode, torch.rand(C, generator=g, dtype=F64) + 1, torch.rand(C, generator=g, dtype=F64) + 0.5, 6.0) if mode else None
    OH, OW = D.out_hw(H, W, stride)
    dy = torch.randn(N, OH, OW, C, generator=g, dtype=F64)
    a = x
    if mode:
        u = x * act[1] + act[2]
        a = u.clamp(0, 6) if mode == 1 else u * torch.sigmoid(u)
    a4, w4, b1 = nchw(a).clone().requires_grad_(), w.view(C, 1, K, K).clone().requires_grad_(), bias.clone().requires_grad_()
    y = F.conv2d(a4, w4, b1, stride=stride, padding=K // 2, groups=C)          # the padding is of the activated tensor
    assert tuple(y.shape) == (N, C, OH, OW)
    da, dw, db = torch.autograd.grad(y, (a4, w4, b1), nchw(dy))
    assert close(D.dw_fwd_ref(x, w, K, stride, act, bias), nhwc(y.detach()))
    assert close(D.dw_dgrad_ref(dy, w, (H, W), K, stride), nhwc(da))
    got_dw, got_db = D.dw_wgrad_ref(x, dy, K, stride, act)
    assert close(got_dw, dw.view(C, K, K)) and close(got_db, db)
    acc = (torch.randn(C, K, K, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64))
    acc_dw, acc_db = D.dw_wgrad_ref(x, dy, K, stride, act, acc)
    assert close(acc_dw, dw.view(C, K, K) + acc[0]) and close(acc_db, db + acc[1])


@pytest.mark.parametrize("case", G.exact_cases(), ids=lambda c: "%s-k%d-s%d-%s" % ("x".join(map(str, c[0])), c[1], c[2], "clamp" if c[3] else "plain"))
def test_integer_cases_of_the_gpu_tests_hold_their_ranges(case):
    shape, K, stride, pro = case
    N, H, W, C = shape
    c = D.dw_case(shape, K, stride, pro)          # asserts: integers, every partial sum <= 256, rows * max|g| * max|a| < 2^24
    assert c["y"].abs().max().item() <= 256 and c["dx"].abs().max().item() <= 256
    for name in ("y", "dx"):
        ref = c[name]
        assert (ref != 0).double().mean().item() >= 0.5, (case, name)
        tile = G.tw_of(H, W) if K == 7 else None
        for kp in (4, 8):
            for region, mask in D.dw_edge_regions(tuple(ref.shape), tile, K, 32 if K == 7 else kp).items():
                assert not bool(mask.any()) or bool((ref[mask] != 0).any()), (case, name, region)
    reach = D.dw_wgrad_ref(torch.ones(shape), torch.ones_like(c["dy"]), K, stride)[0] != 0          # taps that meet the image at all
    assert (c["dw"][reach] != 0).double().mean().item() >= 1 / 3 and not torch.equal(c["dw"], c["dw_acc"]), case
    if pro:          # act(shift) != 0 and both clamps are met: a padding applied before the activation shows
        a = D.dw_activate(c["x"], c["act"])
        assert bool((D.dw_activate(torch.zeros(1, 1, 1, C), c["act"]) != 0).all()) and bool((a == 0).any()) and bool((a == D.HI).any())


def test_weight_gradient_loop_shapes_have_more_tiles_than_workgroups():
    """the premise of the multi-trip cases, restated from pfr_dwconv2d_wgrad_parts: P = min(1024 / ceil(C / 32), tiles)"""
    for N, H, W, C in G.DW7_LOOP_SHAPES:
        tw = G.tw_of(H, W)
        tiles = N * -(-H // tw) * -(-W // tw)
        assert 1024 // -(-C // 32) == 31 and 31 < tiles < 2 * 31          # some workgroups take two trips, the others one


@pytest.mark.parametrize("with_rs", [False, True])
@pytest.mark.parametrize("shape", list(G.LAYER_SCALE_SHAPES))
def test_layer_scale_cases_hold_their_ranges(shape, with_rs):
    c = D.layer_scale_case(shape, with_rs)
    assert (c["y"] != c["res"]).any() and (c["dgamma"] != 0).double().mean().item() >= 0.5
    assert -(-shape[0] * shape[1] // 32) == G.LAYER_SCALE_SHAPES[shape]
    if with_rs and shape[0] > 1:
        assert c["rs"][0].item() == 0 and torch.equal(c["y"][0], c["res"][0])          # a dropped sample


@pytest.mark.parametrize("case", G.real_cases(), ids=lambda c: "%s-k%d-s%d-a%d-%s" % ("x".join(map(str, c[0])), c[1], c[2], c[3], str(c[4])[6:]))
def test_real_valued_cases_of_the_gpu_tests_build(case):
    """the SiLU arguments stay inside the measured sweep, both clamps are met (asserted by the builder); every bound is finite and positive"""
    c = G.real_case(*case)
    for k in ("y_bound", "dx_bound", "dw_bound", "db_bound"):
        assert bool(torch.isfinite(c[k]).all()) and bool((c[k] > 0).all())
    # one rounding of the exact value to the output format is inside the forward bound
    D.assert_within(c["y"].to(case[4]), c["y"], c["y_bound"])


def test_comparison_sees_one_dropped_tap_and_names_its_region():
    """(c) a border tap (the centre tap of the corner pixel) and an interior tap, in both output formats"""
    shape, K = (1, 9, 17, 72), 7
    c = D.dw_case(shape, K)
    for dt in (torch.bfloat16, torch.float32):
        D.dw_assert_exact(c["y"].to(dt), c["y"], "reference against itself", tile=8)
    spatial = ("border ring", "tile-border rows", "tile-border columns", "last ragged tile")
    for drop, regions in (((3, 3, 0, 0), spatial[:3]), ((2, 4, 4, 5), ()), ((0, 0, 8, 16), spatial)):
        broken = D.dw_fwd_ref(c["x"], c["w"], K, 1, None, c["bias"], drop_tap=drop)
        diff = (broken != c["y"])
        assert bool(diff.any()) and not bool(diff[:, :drop[2]].any()) and int(diff.sum((0, 3)).ne(0).sum()) == 1          # that pixel alone
        for dt in (torch.bfloat16, torch.float32):
            with pytest.raises(AssertionError) as e:
                D.dw_assert_exact(broken.to(dt), c["y"], "dropped tap", tile=8)
            msg = str(e.value)
            named = msg.split("mismatches per region")[0]
            assert "(0, %d, %d, " % drop[2:] in msg and all((r in named) == (r in regions) for r in spatial), msg
    # the same at K = 5, stride 2 under the clamp prologue, and in a real-valued case against the per-element bound
    c = D.dw_case((1, 5, 6, 8), 5, 2, True)
    broken = D.dw_fwd_ref(c["x"], c["w"], 5, 2, c["act"], drop_tap=(2, 2, 0, 0))
    with pytest.raises(AssertionError):
        D.dw_assert_exact(broken.bfloat16(), c["y"], "dropped tap", K=5, chunk=8)
    r = G.real_case((1, 9, 17, 72), 7, 1, 0, torch.bfloat16)
    broken = D.dw_fwd_ref(r["x"], r["w"], 7, 1, None, r["bias"], drop_tap=(3, 3, 4, 5))
    D.dw_assert_within(r["y"].bfloat16(), r["y"], r["y_bound"], "one rounding", tile=8)
    with pytest.raises(AssertionError) as e:
        D.dw_assert_within(broken.bfloat16(), r["y"], r["y_bound"], "dropped tap", tile=8)
    assert "(0, 4, 5, " in str(e.value)


def test_edge_regions_of_the_ragged_shape():
    reg = D.dw_edge_regions((2, 9, 17, 72), 8)
    px = lambda m: int(m[0, :, :, 0].sum())
    assert px(reg["border ring"]) == 9 * 17 - 3 * 11
    assert px(reg["tile-border rows"]) == 3 * 17 and px(reg["tile-border columns"]) == 5 * 9          # rows 0 7 8; columns 0 7 8 15 16
    assert px(reg["last ragged tile"]) == 17 + 9 - 1
    assert int(reg["last channel chunk"][0, 0, 0].sum()) == 8 and int(reg["last sample"][:, 0, 0, 0].sum()) == 1
    assert "tile-border rows" not in D.dw_edge_regions((2, 9, 17, 72), None, K=3, chunk=4)
    assert int(D.dw_edge_regions((1, 7, 7, 8), 7)["last ragged tile"].sum()) == 0
