"""Image resampling to another voxel spacing (csrc/resample.hpp): the host plan of the C ABI against the numpy
restatement `resample_ref`, the restatement against properties it does not share code with, the refusals, and the ctypes mirrors of the
new structs.  No GPU needed; tests/test_resample_gpu.py holds the kernels to the restatement bit for bit."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cases
import resample_ref as ref

ROOT = Path(__file__).resolve().parents[1]
geo = cases.geometry

# (N, old spacing, new spacing) -> M, and what the axis exercises
AXES = [
    ((23, 0.9765625, 1.0), 22),   # plain case
    ((17, 0.9765625, 1.0), 17),   # last output edge-clamped
    ((9, 2.5, 1.0), 22),          # 22.5 rounds half to even
    ((3, 2.5, 1.0), 8),           # 7.5 rounds up; one output outside, one edge-clamped
    ((11, 2.0, 1.0), 22),         # last c = 10.5 = N - 0.5 is outside; 11 nearest ties go up
    ((7, 3.0, 1.0), 21),
    ((15, 0.5, 1.25), 6),         # 3 nearest ties
    ((12, 1.0, 2.0), 6),
    ((20, 0.7, 1.0), 14),
    ((13, 1.0, 1.0), 13),         # identity
]


def test_the_axes_exercise_what_they_are_listed_for():
    """The restatement on the listed axes: sizes, the half-to-even rounding, the strict upper bound, the ties of the nearest index."""
    p = {a: ref.plan_axis(*a) for a, _ in AXES}
    for a, m in AXES:
        assert p[a]["M"] == m, a
    q = p[(17, 0.9765625, 1.0)]
    assert q["inside"].all() and q["c"][-1] > 16 and q["base"][-1] == q["next"][-1] == 16
    q = p[(3, 2.5, 1.0)]
    assert list(q["inside"]) == [True] * 7 + [False] and q["c"][6] == 2.4 and q["base"][6] == q["next"][6] == 2
    q = p[(11, 2.0, 1.0)]
    assert q["c"][-1] == 10.5 and not q["inside"][-1] and q["inside"][:-1].all()
    ties = q["c"] + 0.5 == np.floor(q["c"] + 0.5)
    assert np.count_nonzero(ties) == 11 and np.array_equal(q["nearest"][1:-1:2], np.arange(1, 11))  # c = k + 0.5 -> k + 1
    q = p[(15, 0.5, 1.25)]
    assert np.count_nonzero((q["c"] % 1.0) == 0.5) == 3
    q = p[(13, 1.0, 1.0)]
    assert np.array_equal(q["c"], np.arange(13.0)) and not q["frac"].any() and np.array_equal(q["nearest"], np.arange(13))


@pytest.mark.parametrize("axes", [(0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 0, 3), (4, 8, 9)])
def test_plan_of_the_c_abi_equals_the_restatement(engine, axes):
    """mcgpu_resample_plan against plan_axis: integers equal, fractions bit-equal, three listed axes per call."""
    (n, os, ns) = zip(*[AXES[k][0] for k in axes])
    plan = engine.resample_plan(n, os, ns)
    assert plan["shape"] == tuple(AXES[k][1] for k in axes)
    for k in range(3):
        want = ref.plan_axis(n[k], os[k], ns[k])
        for key in ("base", "next", "nearest"):
            assert plan[key][k].dtype == np.int32 and np.array_equal(plan[key][k], want[key]), (key, k)
        assert plan["frac"][k].tobytes() == want["frac"].tobytes(), k
        assert np.array_equal(plan["inside"][k], want["inside"]), k
        assert 0 <= plan["base"][k].min() and plan["next"][k].max() < n[k] and 0 <= plan["nearest"][k].min() and plan["nearest"][k].max() < n[k]


def test_plan_size_alone(engine):
    lib = engine.load_library()
    o = engine._resample_options((23, 17, 9), (0.9765625, 0.9765625, 2.5), (1.0, 1.0, 1.0))
    n_out = (C.c_int * 3)()
    assert lib.mcgpu_resample_plan(C.byref(o), n_out, None, None, None, None, None) == 0
    assert tuple(n_out) == (22, 17, 22)


SHAPE, SPACING, NEW = (11, 9, 7), (2.0, 0.9765625, 2.5), (1.0, 1.0, 1.0)


def _planes(shape, spacing, new_spacing):
    return [ref.plan_axis(n, s, t) for n, s, t in zip(shape, spacing, new_spacing)]


def test_restatement_reproduces_a_ramp():
    """A linear function of the index is reproduced by linear interpolation at every inside voxel whose c <= N - 1 on all axes (beyond
    it the edge value is held)."""
    ca, cb, cc = 3.25, -1.5, 0.875
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in SHAPE], indexing="ij")
    ramp = ca * i + cb * j + cc * k
    got = ref.resample_ref(ramp, SPACING, NEW, "linear", -1000.0, raw=True)
    p = _planes(SHAPE, SPACING, NEW)
    c0, c1, c2 = np.meshgrid(*[q["c"] for q in p], indexing="ij")
    want = ca * c0 + cb * c1 + cc * c2
    sel = np.ones(got.shape, bool)
    for n, c in zip(SHAPE, (c0, c1, c2)):
        sel &= (c >= 0) & (c <= n - 1)
    assert sel.sum() > 0.7 * sel.size and got.shape == (22, 9, 18)
    assert np.all(np.abs(got[sel] - want[sel]) <= 1e-12 * np.maximum(np.abs(want[sel]), 1.0))
    inside = p[0]["inside"][:, None, None] & p[1]["inside"][None, :, None] & p[2]["inside"][None, None, :]
    assert (~inside).any() and np.all(got[~inside] == -1000.0)
    held = inside & ~sel                                   # within half a voxel of the border: the edge value
    edge = ca * np.clip(c0, 0, SHAPE[0] - 1) + cb * np.clip(c1, 0, SHAPE[1] - 1) + cc * np.clip(c2, 0, SHAPE[2] - 1)
    assert held.any() and np.all(np.abs(got[held] - edge[held]) <= 1e-12 * np.maximum(np.abs(edge[held]), 1.0))


def test_restatement_agrees_with_scipy():
    """scipy's order-1 spline with edge replication is the same interpolant at inside voxels (another order of operations: 1e-9)."""
    from scipy import ndimage
    a = np.random.default_rng(5).normal(size=SHAPE) * 100.0
    got = ref.resample_ref(a, SPACING, NEW, "linear", 0.0, raw=True)
    p = _planes(SHAPE, SPACING, NEW)
    coords = np.meshgrid(*[q["c"] for q in p], indexing="ij")
    want = ndimage.map_coordinates(a, coords, order=1, mode="nearest")
    inside = p[0]["inside"][:, None, None] & p[1]["inside"][None, :, None] & p[2]["inside"][None, None, :]
    assert np.all(np.abs(got[inside] - want[inside]) <= 1e-9 * np.maximum(np.abs(want[inside]), 1.0))
    near = ref.resample_ref(a, SPACING, NEW, "nearest", 0.0, raw=True)
    idx = [np.floor(q["c"] + 0.5).astype(int).clip(0, n - 1) for q, n in zip(p, SHAPE)]
    assert np.array_equal(near[inside], a[np.ix_(*idx)][inside])


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32])
@pytest.mark.parametrize("interpolator", ["nearest", "linear"])
def test_restatement_identity_is_bit_exact(dtype, interpolator):
    rng = np.random.default_rng(7)
    a = rng.normal(size=(13, 5, 4)).astype(np.float32) * 300 if dtype is np.float32 else rng.integers(np.iinfo(dtype).min, np.iinfo(dtype).max + 1,
                                                                                                         size=(13, 5, 4)).astype(dtype)
    sp = (0.9765625, 1.0, 2.5)
    out = ref.resample_ref(a, sp, sp, interpolator, -1000.0)
    assert out.dtype == a.dtype and out.shape == a.shape and out.tobytes() == a.tobytes()


def test_restatement_cast_truncates_and_clamps():
    assert ref.cast(-3.5, np.int16) == -3 and ref.cast(3.9, np.int16) == 3 and ref.cast(-0.9, np.int16) == 0
    assert ref.cast(1e6, np.int16) == 32767 and ref.cast(-1e6, np.int16) == -32768
    assert ref.cast(255.9, np.uint8) == 255 and ref.cast(-7.0, np.uint8) == 0 and ref.cast(1e6, np.uint8) == 255
    assert ref.cast(0.1, np.float32) == np.float32(0.1)
    a = np.array([[[-4, -3]]], dtype=np.int16)               # c = 0.5: -4 + 1 * 0.5 = -3.5 -> -3, not -4
    out = ref.resample_ref(a, (1.0, 1.0, 1.0), (1.0, 1.0, 0.5), "linear", 1e6)
    assert out.shape == (1, 1, 4) and list(out.ravel()) == [-4, -3, -3, 32767]  # c = 0, 0.5, 1.0, 1.5 (outside: the default, clamped)


@pytest.mark.parametrize("n, os, ns, what", [
    ((4, 4, 4), (1.0, float("nan"), 1.0), (1.0, 1.0, 1.0), "finite and positive"),
    ((4, 4, 4), (1.0, 1.0, 1.0), (1.0, 0.0, 1.0), "finite and positive"),
    ((4, 4, 4), (1.0, 1.0, -2.0), (1.0, 1.0, 1.0), "finite and positive"),
    ((4, 4, 4), (1.0, 1.0, 1.0), (float("inf"), 1.0, 1.0), "finite and positive"),
    ((4, 1, 4), (1.0, 0.2, 1.0), (1.0, 1.0, 1.0), "rounds to 0"),
    ((4, 0, 4), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), "at least one voxel"),
])
def test_refusals_need_no_device(engine, n, os, ns, what):
    with pytest.raises(engine.EngineError) as e:
        engine.resample_plan(n, os, ns)
    assert e.value.code == -1 and what in e.value.message and "ERROR" in e.value.message


def test_refused_options_and_sizes(engine, case_dir):
    lib = engine.load_library()
    n_out = (C.c_int * 3)()

    def plan(o):
        rc = lib.mcgpu_resample_plan(C.byref(o) if o is not None else None, n_out, None, None, None, None, None)
        return rc, lib.mcgpu_last_error().decode()

    o = engine._resample_options((4, 4, 4), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0))
    assert plan(o)[0] == 0
    o.struct_size = 0
    rc, msg = plan(o)
    assert rc == -1 and "struct_size" in msg
    assert plan(None)[0] == -1
    for field, value in (("dtype", 3), ("dtype", -1), ("interpolator", 2)):
        o = engine._resample_options((4, 4, 4), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0))
        setattr(o, field, value)
        rc, msg = plan(o)
        assert rc == -1 and field in msg, field
    # more than 2^31 - 1 voxels, on the input side and on the output side only
    for n, os in (((2048, 1024, 1024), (1.0, 1.0, 1.0)), ((1024, 1024, 1024), (2.0, 1.0, 1.0))):
        rc, msg = plan(engine._resample_options(n, os, (1.0, 1.0, 1.0)))
        assert rc == -2 and "too large" in msg
    # the entry points that run on a GPU refuse a context without one, and every bad argument before they touch a device
    a = np.zeros((4, 4, 4), np.int16)
    with engine.create(case_dir("water"), device=-1) as ctx:
        for call in (lambda: ctx.resample_volume(a, (1, 1, 1), (2, 2, 2)),
                     lambda: ctx.set_geometry_image_resampled(a, {"body": np.ones(a.shape, np.uint8)}, (1, 1, 1), (2, 2, 2))):
            with pytest.raises(engine.EngineError) as e:
                call()
            assert e.value.code == -1 and "needs a device" in e.value.message
        with pytest.raises(ValueError, match="uint8, int16 or float32"):
            ctx.resample_volume(a.astype(np.float64), (1, 1, 1), (2, 2, 2))
        with pytest.raises(ValueError, match="'linear' or 'nearest'"):
            ctx.resample_volume(a, (1, 1, 1), (2, 2, 2), interpolator="cubic")


def test_ctypes_mirrors_match_the_c_layout(engine, tmp_path):
    """sizeof and every field offset of mcgpu_resample_options / mcgpu_resample_report as a C compiler lays them out from the header."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is needed (the oracle is built with one)"
    structs = {"mcgpu_resample_options": engine.ResampleOptions, "mcgpu_resample_report": engine.ResampleReport}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT / "include" / "mcgpu_amd.h"}"', "int main(void) {"]
    for cname, mirror in structs.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for field, _ in mirror._fields_:
            lines.append(f'  printf("{cname} {field} %zu\\n", offsetof({cname}, {field}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run([cc, "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    seen = 0
    for cname, field, value in re.findall(r"(\w+) (\w+) (\d+)", out):
        mirror = structs[cname]
        assert int(value) == (C.sizeof(mirror) if field == "sizeof" else getattr(mirror, field).offset), (cname, field)
        seen += 1
    assert seen == sum(len(m._fields_) + 1 for m in structs.values())
    header = (ROOT / "include" / "mcgpu_amd.h").read_text()
    assert "#define MCGPU_IMAGE_UINT8 2" in header and engine.IMAGE_UINT8 == 2
    assert engine.load_library().mcgpu_abi_version() == 1  # additions only
    for name in ("mcgpu_resample_plan", "mcgpu_resample_volume", "mcgpu_set_geometry_image_resampled"):
        assert name in engine.ABI_SYMBOLS


def test_python_resampler_without_a_context(tmp_path):
    """`new_spacing=None` hands the input back; anything else needs the GPU: there is no host implementation."""
    a = np.arange(24, dtype=np.int16).reshape(2, 3, 4)
    assert geo.resample_image_spacing(a, (1.0, 1.0, 1.0), None) is a
    with pytest.raises(NotImplementedError, match=r"utils\.py:76-102.*engine_context="):
        geo.resample_image_spacing(a, (1.0, 1.0, 1.0), (2.0, 2.0, 2.0))
    recon = cases.pkg.reconstruction
    recon.write_mha(tmp_path / "ct.mha", a.swapaxes(0, 2), (1.5, 2.0, 2.5), (0.0, 0.0, 0.0), element_type="MET_SHORT")
    with pytest.raises(NotImplementedError, match=r"utils\.py:76-102.*engine_context="):
        geo.load_image_and_segmentations(tmp_path / "ct.mha", image_spacing=(1.0, 1.0, 1.0))
    image, spacing, _ = geo.load_image_and_segmentations(tmp_path / "ct.mha", image_spacing=(1.5, 2.0, 2.5))
    assert spacing == (1.5, 2.0, 2.5) and np.array_equal(image, a)
    with pytest.raises(NotImplementedError, match=r"utils\.py:76-102"):
        geo.MaterialMapperPipeline.create_default_pipeline(body_segmentation=np.ones(a.shape, np.uint8)).execute(a, image_spacing=(1.0, 1.0, 1.0))
