"""The water pre-correction fit without a GPU: the float64 restatement (tests/wpc_ref.py) against the procedure of
the reference's script on an analytic beam-hardened water cylinder, the numpy erosion against scipy's, the water phantom, the weight
and template images and their frame, the C ABI's struct layout and refusals, and what the GPU comparisons leave out.

`centred` (wpc_ref.problem): a water cylinder about the y axis, R = 60 mm, exact chords L, q = -ln(1/2 e^(-0.03 L) + 1/2 e^(-0.015 L)), 40
angles, a centred 64 x 32 detector of 5 mm, volume 40 x 12 x 40 at 4 mm, slab y = 3..7, weight 1 where r < 50 or 70 < r < 78, template
0.02 where r < 60.  In float64: order 1 cond(B) = 47, c = (-0.00161, 1.0310); order 3 cond 1.7e5, residual 2.51e-4 -> 2.23e-6, water
mean r < 20 0.018889 -> 0.019992, 35 < r < 48 0.019670 -> 0.020005; order 5 cond 1.9e9, residual -> 7.8e-7."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cases
import wpc_ref as W
from wpc_ref import fo

pkg = cases.pkg
wp = pkg.water_precorrection
HEADER = Path(__file__).resolve().parents[1] / "include" / "mcgpu_amd.h"


# ---------------------------------------------------------------------------------------------------------------- the rule
def _procedure(p, order, slab):
    """scripts/fit_wpc.py:125-238 on the oracle: whole reconstructions of q^n, the slab cut out of each and averaged, B and a by the
    script's double loop of np.sum, c = inv(B) a."""
    f = [fo.reconstruct(p.proj.astype(np.float64) ** n if n else np.ones(p.proj.shape), *p.geometry_args(), p.dim, p.spacing, p.origin, hann=p.hann,
                        hann_y=p.hann_y, pad=p.pad) for n in range(order + 1)]
    cut = np.index_exp[:, slab[0]: slab[0] + slab[1], :]
    a = np.zeros(order + 1)
    B = np.zeros((order + 1,) * 2)
    for i in range(order + 1):
        fi = f[i][cut].mean(1)
        for j in range(order + 1):
            B[i, j] = np.sum(p.weight * fi * f[j][cut].mean(1))
        a[i] = np.sum(p.weight * fi * p.template)
    return np.linalg.inv(B).dot(a), B


def test_restatement_equals_the_procedure():
    """The restatement (powers by the wpc polynomial e_n, only the slab's slices) against the script's procedure (powers of the
    stack, whole volumes): order-1 coefficients to 1e-6, and they are the ones computed for the issue."""
    p = W.problem("centred")
    want, B_want = _procedure(p, 1, W.CENTRED_SLAB)
    fbar, _ = W.oracle_basis("centred", W.CENTRED_SLAB, 5)
    B, a = W.normal_equations(fbar[:2], p.weight, p.template)
    c = W.solve(B, a)
    assert np.abs(c - want).max() < 1e-6
    assert abs(c[0] + 0.00161) < 5e-6 and abs(c[1] - 1.0310) < 5e-5 and abs(np.linalg.cond(B) - 47.0) < 0.5
    np.testing.assert_allclose(B, B_want, rtol=1e-9)
    np.testing.assert_allclose(wp.solve(B, a), c, rtol=0, atol=0)      # the package's solve is the same statement
    assert wp.residual(c, fbar, p.weight, p.template) == pytest.approx(W.residual(c, fbar, p.weight, p.template), rel=1e-12)


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_the_fit_is_no_worse_than_the_identity(order):
    p = W.problem("centred")
    fbar, _ = W.oracle_basis("centred", W.CENTRED_SLAB, 5)
    B, a = W.normal_equations(fbar[: order + 1], p.weight, p.template)
    c = W.solve(B, a)
    identity = W.unit(1)
    fit, before = W.residual(c, fbar, p.weight, p.template), W.residual(identity, fbar, p.weight, p.template)
    print(f"order {order}: cond(B) = {np.linalg.cond(B):.3g}, residual {before:.3e} -> {fit:.3e}")
    assert fit <= before
    assert before == pytest.approx(2.51e-4, rel=5e-3)
    if order == 3:
        assert fit == pytest.approx(2.23e-6, rel=5e-3) and np.linalg.cond(B) == pytest.approx(1.7e5, rel=0.05)


def test_order_three_flattens_the_water():
    """The cupping of the two-energy beam: 5.6 % and 1.6 % off before, both water regions within 0.1 % of 0.02 after."""
    p = W.problem("centred")
    fbar, _ = W.oracle_basis("centred", W.CENTRED_SLAB, 5)
    B, a = W.normal_equations(fbar[:4], p.weight, p.template)
    image = np.tensordot(W.solve(B, a), fbar[:4], axes=1)
    for region, before in ((p.r < 20.0, 0.018889), ((p.r > 35.0) & (p.r < 48.0), 0.019670)):
        assert fbar[1][region].mean() == pytest.approx(before, abs=5e-7)
        assert abs(image[region].mean() - 0.02) < 1e-3 * 0.02


def test_chords_of_the_cylinder():
    """The analytic input: the central ray crosses 2 R, a ray that passes the axis at distance b crosses 2 sqrt(R^2 - b^2) / cos of its
    tilt, rays outside see nothing; the length cap cuts a steep ray."""
    p = W.problem("centred")
    L = W.cylinder_chords(p, 60.0, 400.0)
    u, v = p.u0 + p.du * np.arange(p.nu), p.v0 + p.dv * np.arange(p.nv)
    iu, iv = 40, 20
    b = 1000.0 * abs(u[iu]) / np.hypot(1500.0, u[iu])                       # distance of the ray's x-z trace from the axis
    tilt = np.hypot(np.hypot(u[iu], 1500.0), v[iv]) / np.hypot(u[iu], 1500.0)
    assert L[iv, iu] == pytest.approx(2.0 * np.sqrt(60.0 ** 2 - b ** 2) * tilt, rel=1e-12)
    assert (L[:, np.abs(u) * 1000.0 / np.hypot(1500.0, u) > 60.0] == 0).all() and L.max() < 2.0 * 60.0 * 1.01
    assert (W.cylinder_chords(p, 60.0, 20.0) < L)[:, 32].any()


# ---------------------------------------------------------------------------------------------------------------- erosion
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_erosion_follows_scipy(k):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(k)
    for shape, fill in (((19, 23, 17), 0.97), ((12, 9, 30), 0.9), ((8, 8, 8), 1.0)):
        mask = rng.uniform(size=shape) < fill   # dense, so that something survives a cube of 8; set voxels touch every border
        assert mask[0].any() and mask[-1].any() and mask[:, 0].any() and mask[:, :, -1].any()
        want = ndi.binary_erosion(mask, structure=np.ones((k,) * 3))
        got = wp.binary_erosion_cube(mask, k)
        assert got.dtype == bool
        np.testing.assert_array_equal(got, want)
    assert k == 1 or not wp.binary_erosion_cube(np.ones((8, 8, 8), bool), k)[0].any()  # outside counts as 0


def test_erosion_window_offsets():
    """Without scipy: a single hole at index i clears exactly the outputs whose window -(k // 2) .. k - 1 - k // 2 contains it."""
    for k in (2, 3, 8):
        line = np.ones(40, bool)
        line[20] = False
        got = wp.binary_erosion_cube(line, k)
        want = np.ones(40, bool)
        for i in range(40):
            window = [i + off for off in range(-(k // 2), k - k // 2)]
            want[i] = all(0 <= j < 40 and line[j] for j in window)
        np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- phantom, weights, frame
def test_water_phantom_geometry():
    g = pkg.geometry.MCWaterPhantomGeometry(shape=(40, 40, 30), image_spacing=(5.0, 5.0, 5.0))
    h2o, air = pkg.materials.material_number("h2o"), pkg.materials.material_number("air")
    x, y = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
    disk = ((x - 20.0) ** 2 + (y - 20.0) ** 2 <= 20.0 ** 2).sum()           # radius 100 mm = 20 voxels about shape / 2
    assert g.materials.shape == (40, 40, 30) and set(np.unique(g.materials)) == {h2o, air} and h2o != air
    assert (g.materials == h2o).sum() == disk * 30                           # length 150 mm = all 30 slices
    assert np.all(g.densities[g.materials == h2o] == np.float32(pkg.geometry.MATERIALS_125KEV["h2o"]))
    assert np.all(g.densities[g.materials == air] == np.float32(pkg.geometry.MATERIALS_125KEV["air"]))
    short = pkg.geometry.MCWaterPhantomGeometry(shape=(40, 40, 30), image_spacing=(5.0, 5.0, 5.0), radius=50.0, length=50.0)
    assert (short.materials == h2o).sum() == ((x - 20.0) ** 2 + (y - 20.0) ** 2 <= 100.0).sum() * 10
    assert (short.materials[:, :, 10:20] == h2o).any() and not (short.materials[:, :, :10] == h2o).any() and not (short.materials[:, :, 20:] == h2o).any()
    with pytest.raises(ValueError):
        pkg.geometry.MCWaterPhantomGeometry(shape=(8, 8, 8), image_spacing=(1.0, 1.0, 2.0))
    full = pkg.geometry.MCWaterPhantomGeometry.__init__.__defaults__
    assert full[0] == (500, 500, 500) and full[1] == (1.0, 1.0, 1.0)


def _script_images(phantom, n_average, erosion, mu_water, mu_air):
    """scripts/fit_wpc.py:162-219 line by line, in the phantom's own [x, y, z] frame: -> (weight, template) averaged over the
    script's z range, [x][y]."""
    h2o, air = pkg.materials.material_number("h2o"), pkg.materials.material_number("air")
    shape = phantom.materials.shape
    water_mask = phantom.materials == h2o
    air_mask = phantom.materials == air
    weight_image = np.zeros_like(phantom.densities, dtype=np.float32)
    weight_image[water_mask] = 1
    if erosion:
        weight_image = wp.binary_erosion_cube(weight_image, erosion).astype(weight_image.dtype)
    weight_image[air_mask] = 1
    x, y, z = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    center = tuple(s / 2 for s in shape)
    fov = ((x - center[0]) ** 2 + (y - center[1]) ** 2 <= (shape[0] / 2) ** 2) & (z >= center[2] - n_average / 2) & (z < center[2] + n_average / 2)
    weight_image = fov * weight_image
    template_image = np.zeros_like(phantom.densities, dtype=np.float32)
    template_image[water_mask] = mu_water
    template_image[air_mask] = mu_air
    mid = shape[-1] // 2
    cut = np.index_exp[..., mid - n_average // 2: mid + n_average // 2]
    return weight_image[cut].mean(-1), template_image[cut].mean(-1)


def test_weight_and_template_follow_the_script():
    """An even number of slices: the slab of the FDK frame is the script's z range.  [x][y] of the phantom is [nx][nz reversed] of
    the volume (IEC X = MC x, IEC Z = -MC y)."""
    phantom = pkg.geometry.MCWaterPhantomGeometry(shape=(40, 36, 30), image_spacing=(5.0, 5.0, 5.0), radius=70.0, length=120.0)
    weight, template, slab = wp.phantom_weight_and_template(phantom, n_average_slices=10, edge_erosion=3, mu_water=0.02, mu_air=1e-5)
    w_xy, t_xy = _script_images(phantom, 10, 3, 0.02, 1e-5)
    assert slab == (10, 10) and weight.shape == template.shape == (36, 40) and weight.dtype == template.dtype == np.float32
    np.testing.assert_array_equal(weight, w_xy.T[::-1])
    np.testing.assert_allclose(template, t_xy.T[::-1], rtol=2e-7, atol=0)  # the script's float32 mean against the float64 mean rounded once
    assert set(np.unique(weight)) == {0.0, 1.0} and (weight == 0).any()
    inner = (weight == 1) & (template == np.float32(0.02))
    rim = (weight == 0) & (template == np.float32(0.02))          # the eroded edge of the water
    assert inner.any() and rim.any() and ((weight == 1) & (template == np.float32(1e-5))).any()
    # defaults: the reference's values
    d = wp.phantom_weight_and_template.__defaults__
    assert d == (50, 8, pkg.defaults.MU_WATER_63KEV, pkg.defaults.MU_AIR_63KEV)
    assert pkg.defaults.MU_WATER_63KEV == 0.02011970928851904 and pkg.defaults.MU_AIR_63KEV == 2.2416145024763944e-05


def test_images_are_in_the_frame_of_prepare_image_for_rtk():
    """A phantom without any symmetry (a box off centre) and no erosion: the template pushed through prepare_image_for_rtk, cut to the
    slab and averaged, is what the function returns; so is a ramp along each axis through to_fdk_frame."""
    h2o, air = pkg.materials.material_number("h2o"), pkg.materials.material_number("air")
    mats = np.full((14, 10, 12), air, np.uint8)
    mats[2:9, 1:4, 3:11] = h2o
    phantom = pkg.geometry.MCGeometry(mats, np.ones(mats.shape, np.float32), (2.0, 2.0, 2.0))
    weight, template, slab = wp.phantom_weight_and_template(phantom, n_average_slices=6, edge_erosion=0, mu_water=0.02, mu_air=0.001)
    volume = np.where(mats == h2o, np.float32(0.02), np.float32(0.001))
    rtk = pkg.forward_projection.prepare_image_for_rtk(volume, input_value_range=None, output_value_range=None, image_spacing=phantom.image_spacing)
    arr = rtk.array
    assert arr.shape == (10, 12, 14) and slab == (3, 6)
    np.testing.assert_array_equal(template, arr[:, 3:9, :].mean(1, dtype=np.float64).astype(np.float32))
    np.testing.assert_array_equal(wp.to_fdk_frame(volume), arr)
    x, y, z = np.meshgrid(np.arange(14), np.arange(10), np.arange(12), indexing="ij")
    np.testing.assert_array_equal(wp.to_fdk_frame(x)[4, 5, :], np.arange(14))            # IEC X = MC x
    np.testing.assert_array_equal(wp.to_fdk_frame(z)[4, :, 5], np.arange(12)[::-1])      # IEC Y = -MC z
    np.testing.assert_array_equal(wp.to_fdk_frame(y)[:, 5, 5], np.arange(10)[::-1])      # IEC Z = -MC y
    assert weight.shape == (10, 14)


@pytest.mark.parametrize("nz, n, want", [(30, 10, (10, 10)), (31, 10, (10, 10)), (30, 7, (12, 6)), (250, 50, (100, 50)), (13, 12, (0, 12))])
def test_slab_for_even_and_odd_sizes(nz, n, want):
    h2o = pkg.materials.material_number("h2o")
    phantom = pkg.geometry.MCGeometry(np.full((6, 6, nz), h2o, np.uint8), np.ones((6, 6, nz), np.float32), (1.0, 1.0, 1.0))
    assert wp.phantom_weight_and_template(phantom, n_average_slices=n, edge_erosion=0)[2] == want
    assert want == (nz // 2 - n // 2, 2 * (n // 2))


def test_slab_that_does_not_fit_is_refused():
    h2o = pkg.materials.material_number("h2o")
    phantom = pkg.geometry.MCGeometry(np.full((6, 6, 8), h2o, np.uint8), np.ones((6, 6, 8), np.float32), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        wp.phantom_weight_and_template(phantom, n_average_slices=12, edge_erosion=0)


# ---------------------------------------------------------------------------------------------------------------- what the GPU tests leave out
@pytest.mark.parametrize("name, slab, order", W.GPU_CASES)
def test_gpu_comparisons_leave_out_at_most_five_percent(name, slab, order):
    """A pixel is left out when a voxel of its slab column is within 1e-3 pixel of a detector edge in some projection."""
    p = W.problem(name)
    assert 0 <= slab[0] and slab[0] + slab[1] <= p.dim[1]
    share = W.problem(name).left_out(slab).mean()
    print(f"{name} slab {slab}: {100 * share:.2f} % of the pixels left out")
    assert share <= 0.05


def test_gpu_cases_reach_the_launch_shapes():
    assert W.problem("half_fan").n == 41 and W.problem("half_fan").n % 32 == 9 and 41 % 8 == 1     # chunks 32 + 9, a last batch of one
    assert W.problem("centred").n == 40                                                              # chunks 32 + 8
    assert W.problem("wide").dim[0] == 300 and W.problem("wide").dim[1] == 1 and W.problem("wide").origin is not None
    vo = W.problem("varying_offsets").geo
    assert np.ptp(vo.projection_offsets_x) > 5.0 and np.ptp(vo.projection_offsets_y) > 2.0
    assert {s for n, s, _ in W.GPU_CASES if n == "half_fan"} == {(0, 1), (0, 30), (27, 3)}


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def _header_fields(struct):
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S)
    assert body, struct
    names = []
    for decl in body.group(1).split(";"):
        parts = [re.sub(r"\[.*?\]", "", p).replace("*", " ").split() for p in decl.split(",")]
        if parts[0]:
            names += [parts[0][-1]] + [p[0] for p in parts[1:]]
    return names


def test_ctypes_mirrors_match_the_c_layout(tmp_path):
    """Field names in the header's order; sizeof and every offsetof / size as the C compiler lays the header out."""
    mirrors = [("mcgpu_wpc_fit_options", wp._WpcFitOptions), ("mcgpu_wpc_fit_report", wp._WpcFitReport)]
    for struct, cls in mirrors:
        assert _header_fields(struct) == [f[0] for f in cls._fields_], struct
    cc = next((shutil.which(c) for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "mcgpu_amd.h"', "int main(void) {"]
    for struct, cls in mirrors:
        lines.append(f'  printf("{struct} %zu\\n", sizeof({struct}));')
        for name, _ in cls._fields_:
            lines.append(f'  printf("{struct}.{name} %zu %zu\\n", offsetof({struct}, {name}), sizeof((({struct} *)0)->{name}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-I", str(HEADER.parent), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    c_side = dict(line.split(" ", 1) for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    py_side = {}
    for struct, cls in mirrors:
        py_side[struct] = str(C.sizeof(cls))
        for name, _ in cls._fields_:
            f = getattr(cls, name)
            py_side[f"{struct}.{name}"] = f"{f.offset} {f.size}"
    assert c_side == py_side
    # the FDK fields sit where mcgpu_fdk_options has them, up to hann_y
    fdk = pkg.reconstruction._FdkOptions
    for name, _ in fdk._fields_[: [f[0] for f in fdk._fields_].index("wpc")]:
        assert getattr(fdk, name).offset == getattr(wp._WpcFitOptions, name).offset, name


class _Tiny:
    """mcgpu_wpc_fit through ctypes on the smallest valid problem; keyword arguments replace fields of the options."""

    def __init__(self):
        self.lib = pkg.engine.load_library()
        self.lib.mcgpu_wpc_fit.argtypes = [C.POINTER(wp._WpcFitOptions)] + [C.c_void_p] * 6 + [C.POINTER(wp._WpcFitReport)]
        self.lib.mcgpu_wpc_fit.restype = C.c_int
        self.angle = np.array([30.0])
        self.arrays = dict(projections=np.array([[[1.0, 2.0], [3.0, 4.0]]], np.float32), weight=np.ones((1, 1), np.float32),
                           template_=np.ones((1, 1), np.float32), B=np.full((2, 2), -1.0), a=np.full(2, -1.0))

    def options(self, **fields):
        o = wp._WpcFitOptions(C.sizeof(wp._WpcFitOptions), 1, 2, 2, 4.0, 4.0, -2.0, -2.0, 1000.0, 1500.0, self.angle.ctypes.data_as(C.POINTER(C.c_double)),
                              None, None, 1, 3, 1, 1.0, 1.0, 1.0, *(float("nan"),) * 3, 0.0, 0.0, 0.0, 1, 0, 1, 0, 0)
        for k, v in fields.items():
            setattr(o, k, v)
        return o

    def __call__(self, o, missing=None):
        ptr = [None if k == missing else v.ctypes.data for k, v in self.arrays.items()]
        rc = self.lib.mcgpu_wpc_fit(C.byref(o) if o is not None else None, *ptr, None, None)
        untouched = np.all(self.arrays["B"] == -1.0) and np.all(self.arrays["a"] == -1.0)
        return rc, untouched, self.lib.mcgpu_last_error().decode(errors="replace")


_SET_SIZE = "!!ERROR!! mcgpu_wpc_fit: set mcgpu_wpc_fit_options.struct_size = sizeof(mcgpu_wpc_fit_options)"
_NULL = C.POINTER(C.c_double)()
REFUSALS = [
    ("options", None, None, _SET_SIZE),
    ("struct_size", dict(struct_size=0), None, _SET_SIZE),
    ("projections", {}, "projections", "!!ERROR!! mcgpu_wpc_fit: null pointer: projections"),
    ("weight", {}, "weight", "!!ERROR!! mcgpu_wpc_fit: null pointer: weight"),
    ("template", {}, "template_", "!!ERROR!! mcgpu_wpc_fit: null pointer: template_"),
    ("B", {}, "B", "!!ERROR!! mcgpu_wpc_fit: null pointer: B"),
    ("a", {}, "a", "!!ERROR!! mcgpu_wpc_fit: null pointer: a"),
    ("order_0", dict(order=0), None, "!!ERROR!! mcgpu_wpc_fit: order 0 is outside 1..7"),
    ("order_8", dict(order=8), None, "!!ERROR!! mcgpu_wpc_fit: order 8 is outside 1..7"),
    ("y_count_0", dict(y_count=0), None, "!!ERROR!! mcgpu_wpc_fit: y_count 0 is below 1"),
    ("y_count_negative", dict(y_count=-2), None, "!!ERROR!! mcgpu_wpc_fit: y_count -2 is below 1"),
    ("slab_before", dict(y_first=-1), None, "!!ERROR!! mcgpu_wpc_fit: the slab [-1, 0) is outside [0, 3)"),
    ("slab_beyond", dict(y_first=2, y_count=2), None, "!!ERROR!! mcgpu_wpc_fit: the slab [2, 4) is outside [0, 3)"),
    ("slab_overflow", dict(y_first=2, y_count=2 ** 31 - 1), None, "!!ERROR!! mcgpu_wpc_fit: the slab [2, 2147483649) is outside [0, 3)"),
    ("n_proj", dict(n_proj=0), None, "bad FDK argument (n_proj 0,"),
    ("nu", dict(nu=1), None, "bad FDK argument (n_proj 1, nu 1,"),
    ("du", dict(du=0.0), None, "du 0.000000"),
    ("ny", dict(ny=0), None, "volume 1 x 0 x 1"),
    ("gantry_deg", dict(gantry_deg=_NULL), None, "gantry_deg NULL)"),
    ("layout", dict(channel_layout=3), None, "!!ERROR!! mcgpu_wpc_fit: channel_layout 3 is outside 0..2"),
]


@pytest.mark.parametrize("what, fields, missing, message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_abi_refuses_before_any_hip_call(engine, what, fields, missing, message):
    """-1 and the message with the value in it, B and a untouched; runs without a device, so nothing of HIP was asked."""
    call = _Tiny()
    rc, untouched, msg = call(None if fields is None else call.options(**fields), missing)
    assert rc == -1 and untouched
    assert msg.startswith("!!ERROR!! mcgpu_wpc_fit: ") and message in msg and (msg == message or not message.startswith("!!"))


def test_abi_a_device_that_does_not_exist_is_an_error_return(engine):
    call = _Tiny()
    rc, untouched, msg = call(call.options(device=9999))
    assert rc == -1 and untouched and "!!HIP ERROR!! hipSetDevice" in msg


def test_python_checks_its_arguments_before_the_library():
    p = W.problem("centred")
    with pytest.raises(ValueError, match="slab means"):
        wp.fit_wpc(*p.fdk_args(), p.weight[:-1], p.template, W.CENTRED_SLAB, order=1, pad=0.0)
    with pytest.raises(ValueError, match="geometry entries"):
        wp.fit_wpc(p.proj[:-1], *p.fdk_args()[1:], p.weight, p.template, W.CENTRED_SLAB, order=1, pad=0.0)
