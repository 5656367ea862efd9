"""The resampling rule of DESIGN.md row f12 / csrc/resample.hpp restated in numpy float64, for the tests: written from the rule's
text, not from the kernel.  SimpleITK's Resample with the identity transform, origin and direction unchanged, as the reference's
`resample_image_spacing` (cbctmc/utils.py:76-102) calls it; arrays are [n0][n1][n2] with one spacing per array axis.

Every operation is one IEEE double operation on whole arrays (numpy never fuses a multiply and an add), in the rule's order."""
import numpy as np

_RANGE = {np.dtype(np.int16): (-32768.0, 32767.0), np.dtype(np.uint8): (0.0, 255.0)}


def plan_axis(N, os, ns):
    """One axis of the rule: dict(M, c, inside, nearest, base, next, frac) for input size N, old spacing os, new spacing ns."""
    N, os, ns = int(N), float(os), float(ns)
    M = int(round(N * (os / ns)))                      # Python's round: half to even
    i = np.arange(M, dtype=np.float64)
    c = (i * ns) / os
    inside = (c >= -0.5) & (c < N - 0.5)               # the upper bound is strict
    nearest = np.clip(np.floor(c + 0.5), 0, N - 1)     # RoundHalfIntegerUp; clamped into the axis, which changes it outside only
    base = np.clip(np.floor(c), 0, N - 1)
    nxt = np.minimum(base + 1, N - 1)
    frac = np.maximum(c - base, 0.0)
    return {"M": M, "c": c, "inside": inside, "nearest": nearest.astype(np.int32), "base": base.astype(np.int32), "next": nxt.astype(np.int32),
            "frac": frac}


def cast(values, dtype):
    """double -> `dtype` as the rule casts: float32 rounds to nearest; int16 / uint8 clamp to the range, then truncate toward zero (a
    NaN becomes 0)."""
    dtype = np.dtype(dtype)
    v = np.asarray(values, dtype=np.float64)
    if dtype == np.float32:
        return v.astype(np.float32)
    lo, hi = _RANGE[dtype]
    v = np.where(np.isnan(v), 0.0, v)
    return np.trunc(np.minimum(np.maximum(v, lo), hi)).astype(dtype)


def _lerp(a, b, d):
    return a + (b - a) * d


def resample_ref(array, spacing, new_spacing, interpolator="linear", default=0.0, raw=False):
    """`array` resampled from `spacing` to `new_spacing` by the rule; the element type stays.  raw=True: the float64 values before
    the cast (the default value uncast too)."""
    a = np.asarray(array)
    assert a.ndim == 3
    p = [plan_axis(n, s, t) for n, s, t in zip(a.shape, spacing, new_spacing)]
    if any(q["M"] < 1 for q in p):
        raise ValueError("an axis rounds to 0 voxels")
    inside = p[0]["inside"][:, None, None] & p[1]["inside"][None, :, None] & p[2]["inside"][None, None, :]
    if interpolator == "nearest":
        values = a[np.ix_(p[0]["nearest"], p[1]["nearest"], p[2]["nearest"])]
        if raw:
            return np.where(inside, values.astype(np.float64), float(default))
        return np.where(inside, values, cast(default, a.dtype))
    assert interpolator == "linear"
    f = a.astype(np.float64)

    def taps(k0, k1, k2):
        return f[np.ix_(p[0][k0], p[1][k1], p[2][k2])]

    d0, d1, d2 = p[0]["frac"][:, None, None], p[1]["frac"][None, :, None], p[2]["frac"][None, None, :]
    # along the last axis (x of the image handed to SimpleITK), then the middle one, then the first
    x00 = _lerp(taps("base", "base", "base"), taps("base", "base", "next"), d2)
    x01 = _lerp(taps("base", "next", "base"), taps("base", "next", "next"), d2)
    x10 = _lerp(taps("next", "base", "base"), taps("next", "base", "next"), d2)
    x11 = _lerp(taps("next", "next", "base"), taps("next", "next", "next"), d2)
    values = _lerp(_lerp(x00, x01, d1), _lerp(x10, x11, d1), d0)
    if raw:
        return np.where(inside, values, float(default))
    return np.where(inside, cast(values, a.dtype), cast(default, a.dtype))
