"""Shared by tests/test_overviews.py and tests/test_gpu_overviews.py: the NumPy float32 model of one overview level
(the contract of csrc/overview.hpp) and the value mix the levels are checked on."""
import numpy as np

import pcr

NAN_BITS = np.uint32(0x7FC00000)


def down(src, mode="average"):
    """One level: ceil(h/2) x ceil(w/2); cells outside the source and NaN cells are invalid."""
    h, w = src.shape
    p = np.full((2 * ((h + 1) // 2), 2 * ((w + 1) // 2)), np.nan, np.float32)
    p[:h, :w] = src
    q = [p[0::2, 0::2], p[0::2, 1::2], p[1::2, 0::2], p[1::2, 1::2]]
    if mode == "nearest":
        return q[0].copy()
    v = [~np.isnan(x) for x in q]
    a, b, c, d = [np.where(m, x, np.float32(0.0)) for m, x in zip(v, q)]
    with np.errstate(all="ignore"):
        out = (((a + b) + c) + d) / (v[0].astype(np.float32) + v[1] + v[2] + v[3]).astype(np.float32)
    out.view(np.uint32)[np.isnan(out)] = NAN_BITS          # n == 0 and Inf + -Inf: one NaN on every machine
    return out


def pyramid(src, levels, mode="average"):
    out = []
    for _ in range(levels):
        src = down(src, mode)
        out.append(src)
    return out


def max_levels(w, h):
    k = 0
    while w > 1 or h > 1:
        w, h, k = (w + 1) // 2, (h + 1) // 2, k + 1
    return k


def bits_equal(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (f"{what}: {int(bad.sum())} cells differ bitwise, first at {np.argwhere(bad)[:3].tolist()}: "
                           f"{got.view(np.uint32)[bad][:3]} != {want.view(np.uint32)[bad][:3]}")


def values(w, h, seed, nan_fraction=0.2):
    """(h, w) float32: normal values of many magnitudes up to FLT_MAX (sums overflow to Inf), denormals, +-Inf (some in one
    window: Inf + -Inf), -0.0, and NaNs of several payloads (nearest copies them)."""
    rng = np.random.default_rng(seed)
    n = w * h
    a = (rng.normal(0.0, 1.0, n) * 10.0 ** rng.integers(-3, 6, n)).astype(np.float32)
    kind = rng.uniform(size=n)
    fmax = np.finfo(np.float32).max
    a[kind < 0.04] = rng.choice(np.array([fmax, -fmax, fmax / 2, fmax / 3], np.float32), int((kind < 0.04).sum()))
    a[(kind >= 0.04) & (kind < 0.07)] = rng.choice(np.array([np.inf, -np.inf], np.float32), int(((kind >= 0.04) & (kind < 0.07)).sum()))
    a[(kind >= 0.07) & (kind < 0.10)] = np.float32(-0.0)
    den = (kind >= 0.10) & (kind < 0.13)
    a[den] = rng.integers(1, 1 << 23, int(den.sum())).astype(np.uint32).view(np.float32) * rng.choice([-1, 1], int(den.sum())).astype(np.float32)
    nan = rng.uniform(size=n) < nan_fraction
    a.view(np.uint32)[nan] = rng.choice(np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0x7F800001], np.uint32), int(nan.sum()))
    return a.reshape(h, w)


def make_grid(arrays, names=None):
    h, w = arrays[0].shape
    bands = []
    for i in range(len(arrays)):
        b = pcr.BandDesc()
        b.name = names[i] if names else f"band{i}"
        bands.append(b)
    g = pcr.Grid.create(w, h, bands)
    for i, a in enumerate(arrays):
        g.set_band_array(i, a)
        bits_equal(np.array(g.band_array(i)), a, "set_band_array keeps bits")
    return g


def grid_bands(g):
    return [np.array(g.band_array(b)) for b in range(g.num_bands())]
