"""ptsvgf.skin: the weights and bones of a bending chain."""
import numpy as np
import pytest

from ptsvgf import skin


def _positions(n=5000, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 3)).astype(np.float32)


BASE, TIP = (0.125, -0.5, 0.25), (0.125, 0.75, 0.25)  # exact in float32: the ends are hit exactly


@pytest.mark.parametrize("n_bones", [1, 2, 4, 8])
def test_chain_weights(n_bones):
    p = _positions()
    p[0], p[1] = BASE, TIP
    b, w = skin.chain_weights(p, BASE, TIP, n_bones)
    assert b.shape == w.shape == (len(p), 4) and b.dtype == np.uint16 and w.dtype == np.float32
    assert b.max() <= n_bones - 1 and np.all(w >= 0)
    total = w[:, 0] + w[:, 1] + w[:, 2] + w[:, 3]  # float32 sums
    assert np.max(np.abs(total - np.float32(1.0))) <= np.spacing(np.float32(1.0))
    assert np.all(np.count_nonzero(w, axis=1) <= 2)
    assert np.all(w[:, 2:] == 0) and np.all(b[:, 2:] == 0)
    if n_bones == 1:
        assert np.all(b == 0) and np.all(w[:, 0] == 1)
        return
    assert np.all(b[:, 1] == b[:, 0] + 1)
    # the ends: the base follows bone 0 alone, the tip the last bone alone; beyond them the parameter is clamped
    assert w[0, 0] == 1 and b[0, 0] == 0
    assert w[1, 1] == 1 and b[1, 1] == n_bones - 1
    below, above = p[:, 1] <= BASE[1], p[:, 1] >= TIP[1]
    assert below.any() and above.any()
    assert np.all(w[below, 0] == 1) and np.all(b[below, 0] == 0)
    assert np.all(w[above, 1] == 1) and np.all(b[above, 1] == n_bones - 1)
    # the parameter: s (n_bones - 1) = i + f
    s = np.clip((p[:, 1].astype(np.float64) - BASE[1]) / (TIP[1] - BASE[1]), 0, 1)
    assert np.max(np.abs(b[:, 0] + w[:, 1].astype(np.float64) - s * (n_bones - 1))) <= 1e-6


def test_chain_weights_mask_and_shared_vertices():
    p = _positions(seed=1)
    mask = np.arange(len(p)) % 3 != 0
    b, w = skin.chain_weights(p, BASE, TIP, 8, mask)
    assert np.all(w[~mask] == 0) and np.all(b[~mask] == 0)
    assert np.all(w[mask].sum(axis=1) > 0.99)
    # a function of the position alone: the same vertex in another list gets the same influences
    perm = np.random.default_rng(2).permutation(len(p))
    b2, w2 = skin.chain_weights(p[perm], BASE, TIP, 8, mask[perm])
    assert np.array_equal(b2, b[perm]) and np.array_equal(w2.view(np.uint32), w[perm].view(np.uint32))


def test_corner_positions():
    rng = np.random.default_rng(3)
    tri = rng.uniform(-1, 1, (10, 45)).astype(np.float32)
    cp = skin.corner_positions(tri)
    assert cp.shape == (30, 3) and np.array_equal(cp[4], tri[1, 3:6])
    raster = rng.uniform(-1, 1, 10 * 18).astype(np.float32)
    rp = skin.corner_positions_raster(raster)
    assert rp.shape == (30, 3) and np.array_equal(rp[4], raster[24:27])


@pytest.mark.parametrize("n_bones", [1, 2, 8])
def test_chain_bones(n_bones):
    ident = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (n_bones, 1))
    zero = skin.chain_bones(BASE, TIP, n_bones, 0.0, (0, 0, 1))
    assert zero.dtype == np.float32 and np.array_equal(zero.view(np.uint32), ident.view(np.uint32))
    for bend in (-25.0, 8.0, 90.0):
        m = skin.chain_bones(BASE, TIP, n_bones, bend, (0, 0, 1))
        assert m.shape == (n_bones, 16)
        assert np.array_equal(m[0].view(np.uint32), ident[0].view(np.uint32))  # bone 0: the identity for any bend
        M = m.astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)
        assert np.all(M[:, 3] == (0, 0, 0, 1))
        for i in range(1, n_bones):
            # rigid, turned by i steps about z, and continuous at its joint with the bone before
            R = M[i, :3, :3]
            assert np.max(np.abs(R @ R.T - np.eye(3))) <= 1e-6 and abs(np.linalg.det(R) - 1) <= 1e-6
            ang = np.degrees(np.arctan2(R[1, 0], R[0, 0]))
            assert abs(ang - bend * i / (n_bones - 1)) <= 1e-4
            joint = np.append(np.asarray(BASE) + (np.asarray(TIP) - BASE) * i / (n_bones - 1), 1.0)
            assert np.max(np.abs(M[i] @ joint - M[i - 1] @ joint)) <= 1e-6
