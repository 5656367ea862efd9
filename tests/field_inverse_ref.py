"""The field inversion of DESIGN.md row f22 restated in numpy: the rule in the header of csrc/field_inverse.hip, operation by operation.
Every function takes `dtype`: float64 is the reference, float32 is the same code in the kernels' precision (its error against the float64
run is the yardstick for the kernels).  The sampler is registration_ref's.

Fields are [3, x, y, z] in voxels, component i along axis i.  The inverse v of u satisfies u(x + v(x)) + v(x) ~ 0."""
from __future__ import annotations

import numpy as np

from registration_ref import _grid, sample


def residual(u, v, dtype=np.float64):
    """r_i(x) = v_i(x) + u_i at c = x + v(x): one set of coordinates for the three components."""
    u, v = np.asarray(u, dtype=dtype), np.asarray(v, dtype=dtype)
    g = _grid(v.shape[1:], dtype)
    coords = [g[i] + v[i] for i in range(3)]
    return np.stack([v[i] + sample(u[i], coords, dtype) for i in range(3)])


def step(u, v, relaxation, dtype=np.float64):
    """v_i - w r_i: a product, then a difference; every tap reads the old v (Jacobi)."""
    v = np.asarray(v, dtype=dtype)
    return v - dtype(relaxation) * residual(u, v, dtype)


def norms(r):
    """(max |r_i(x)|, sqrt(sum double(r_i)^2 / (3 N)))."""
    r = np.asarray(r).astype(np.float64)
    return float(np.abs(r).max()), float(np.sqrt((r * r).sum() / r.size))


def invert(u, iterations=40, relaxation=0.5, initial=None, dtype=np.float64):
    """-> (v in dtype, report dict with iterations and residual_max / residual_rms before and after).  No early stop."""
    u = np.asarray(u, dtype=dtype)
    v = np.zeros_like(u) if initial is None else np.array(initial, dtype=dtype)
    report = dict(iterations=int(iterations))
    report["residual_max_before"], report["residual_rms_before"] = norms(residual(u, v, dtype))
    for _ in range(int(iterations)):
        v = step(u, v, relaxation, dtype)
    report["residual_max_after"], report["residual_rms_after"] = norms(residual(u, v, dtype))
    return v, report


def as_invert_field(dtype=np.float64, calls=None):
    """The restatement with the signature `CorrespondenceModel.inverted(_invert=...)` calls: -> (float32 field, report)."""
    def invert_field(field, iterations=40, relaxation=0.5, initial=None, gpu_id=0):
        if calls is not None:
            calls.append(dict(iterations=iterations, relaxation=relaxation, gpu_id=gpu_id))
        v, report = invert(field, iterations, relaxation, initial, dtype)
        return v.astype(np.float32), report
    return invert_field


# the five-phase fixture of the model tests: a sphere of radius 5 on (24, 20, 16) at z = 9 - 2 a, reference phase 2
PHASE_SHAPE = (24, 20, 16)
PHASE_SIGNALS = np.array([[0.0, 0.5], [0.6, 0.4], [1.0, 0.0], [0.6, -0.4], [0.0, -0.5]])
PHASE_REGISTRATION = dict(iterations=60, n_levels=2)


def phase_images():
    from registration_ref import sphere
    return np.stack([sphere(PHASE_SHAPE, (12, 10, 9 - 2.0 * a), 5.0) for a in PHASE_SIGNALS[:, 0]])
