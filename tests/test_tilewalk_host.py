"""The tile queue of the pair entry points (csrc/pfr_tilewalk.h) through pfr_pair_tile_coords, no GPU: the decode the kernels run —
the double-precision sqrt guess of the triangle and its two fix-up loops included — against a plain enumeration, and at the largest
geometry the contract allows."""
import numpy as np
import pytest
import torch

T, SUPER = 128, 16


def _coords(t0, n, Na, Nb, sym):
    from pets_face_recognition_amd._hip import lib
    out = torch.full((n, 2), -7, dtype=torch.int32)
    lib.pfr_pair_tile_coords(t0, n, Na, Nb, 1 if sym else 0, out.data_ptr())
    return out.numpy()


def _enumerate(Na, Nb, sym):
    """super-tiles row-major (symmetric: column >= row only), the 256 tiles of one row-major; -1, -1 where a slot holds no tile"""
    ntm, ntn = -(-Na // T), -(-Nb // T)
    nsm, nsn = -(-ntm // SUPER), -(-ntn // SUPER)
    out = []
    for sm in range(nsm):
        for sn in range(sm if sym else 0, nsn):
            for l in range(SUPER * SUPER):
                tm, tn = sm * SUPER + l // SUPER, sn * SUPER + l % SUPER
                out.append((tm, tn) if tm < ntm and tn < ntn and (not sym or tn >= tm) else (-1, -1))
    return np.array(out, dtype=np.int32), ntm, ntn


def _check(Na, Nb, sym):
    want, ntm, ntn = _enumerate(Na, Nb, sym)
    got = _coords(0, len(want), Na, Nb, sym)
    assert np.array_equal(got, want), (Na, Nb, sym)                  # the order and the skipped slots
    tiles = [tuple(x) for x in got if x[0] >= 0]
    assert len(tiles) == len(set(tiles)) == (ntn * (ntn + 1) // 2 if sym else ntm * ntn)     # every tile exactly once
    assert all(0 <= a < ntm and 0 <= b < ntn and (not sym or b >= a) for a, b in tiles)


@pytest.mark.parametrize("sym", [True, False])
def test_every_tile_once_in_order_for_1_to_80_tiles(sym):
    for n in range(1, 81):                                            # 1 .. 5 super-tiles per side
        _check(T * n, T * n, sym)


def test_ragged_rectangles_and_ragged_triangles():
    for Na, Nb in [(2049, 130), (130, 2049), (1, 1), (129, 128), (2048, 2049), (4097, 2047)]:
        _check(Na, Nb, False)
    for N in [2, 129, 2049, 4097, 6145]:
        _check(N, N, True)


def test_a_window_of_the_queue_equals_the_whole():
    want, _, _ = _enumerate(T * 40, T * 40, True)
    assert len(want) == 6 * 256                                       # 3 super-tiles per side: 6 in the triangle
    assert np.array_equal(_coords(700, 800, T * 40, T * 40, True), want[700:1500])
    assert _coords(5, 0, T * 40, T * 40, True).shape == (0, 2)


def test_the_largest_geometry():
    """Na = 2^31 - 1, symmetric: 2^24 tiles and ns = 2^20 super-tiles per side, 2^39 + 2^19 super-tiles.  Row r of the super-tile triangle
    starts at su = r ns - r (r - 1) / 2: its first slot is tile (16 r, 16 r), the slot before it is the last tile of row r - 1's last
    super-tile, (16 r - 1, 2^24 - 1) — where a sqrt guess that is off by one lands in the wrong row."""
    N, ns, nt = 2 ** 31 - 1, 2 ** 20, 2 ** 24
    nsuper = ns * (ns + 1) // 2
    assert _coords(0, 1, N, N, True).tolist() == [[0, 0]]
    assert _coords(nsuper * 256 - 1, 1, N, N, True).tolist() == [[nt - 1, nt - 1]]
    for r in [1, 2, 3, 1000, 2 ** 19 - 1, 2 ** 19, 2 ** 19 + 1, 777777, ns - 3, ns - 2, ns - 1]:
        t = (r * ns - r * (r - 1) // 2) * 256
        got = _coords(t - 1, 2, N, N, True).tolist()
        assert got == [[16 * r - 1, nt - 1], [16 * r, 16 * r]], (r, got)
    # inside a row: super-tile (r, r + 5), tile 17 of it (row 1, column 1)
    r = 2 ** 19
    t = (r * ns - r * (r - 1) // 2 + 5) * 256 + 17
    assert _coords(t, 1, N, N, True).tolist() == [[16 * r + 1, 16 * (r + 5) + 1]]


def test_refusals():
    from pets_face_recognition_amd._hip import PfrError
    with pytest.raises(PfrError, match="not inside the queue"):
        _coords(0, 257, 128, 128, True)
    with pytest.raises(PfrError, match="not inside the queue"):
        _coords(-1, 1, 128, 128, False)
    with pytest.raises(PfrError, match="must be >= 1"):
        _coords(0, 1, 0, 128, False)
    with pytest.raises(PfrError, match="equal in symmetric mode"):
        _coords(0, 1, 128, 256, True)
