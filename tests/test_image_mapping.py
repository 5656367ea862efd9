"""CT image + segmentations -> (material, density): the host statement of the mapping rule (csrc/image_map.hpp) in
`geometry.py` -- mapper classes, `MaterialMapperPipeline`, `MCGeometry.from_image` -- its closed form, the `.mha` element types it reads
and the ctypes mirrors of the new C structs.  No GPU needed; tests/test_image_mapping_gpu.py holds the device to the same arrays."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cases

ROOT = Path(__file__).resolve().parents[1]
geo = cases.geometry
recon = cases.pkg.reconstruction
num = cases.materials.material_number
RHO = {k: np.float32(v) for k, v in cases.materials.MATERIALS_125KEV.items()}


def _execute(image, **segmentations):
    return geo.MaterialMapperPipeline.create_default_pipeline(**{f"{k}_segmentation": v for k, v in segmentations.items()}).execute(image)


def _names(materials):
    return np.array(cases.materials.MATERIAL_IDS, dtype=object)[materials.astype(int) - 1]


def test_bone_cube_known_answer():
    """A 5 x 5 x 5 bone cube whose +x face lies on the volume border, HU on both sides of 150 and 300: below 150 red_marrow, [150, 300)
    bone_020, from 300 bone_050 in the 3 x 3 x 3 core and bone_100 on the one-voxel outline -- the face on the border included, because
    voxels outside the volume count as background."""
    shape = (8, 9, 9)
    body = np.ones(shape, np.uint8)
    bone = np.zeros(shape, np.uint8)
    bone[3:8, 2:7, 2:7] = 1                      # x = 7 is the last index: that face touches the border
    image = np.full(shape, 400, np.int16)
    image[:, :, 2] = 149                         # one z layer of the cube: marrow
    image[:, :, 3] = 150                         # bone_020 from exactly 150 ...
    image[:, 2, 4] = 299                         # ... to just below 300
    image[:, 3, 4] = 300                         # bone_050 / bone_100 from exactly 300
    m, d = _execute(image, body=body, bone=bone)
    want = np.full(shape, "soft_tissue", dtype=object)
    core = np.zeros(shape, bool)
    core[4:7, 3:6, 3:6] = True                   # the erosion of the cube -- NOT up to x = 7
    cube = bone > 0
    want[cube & (image < 150)] = "red_marrow"
    want[cube & (image >= 150) & (image < 300)] = "bone_020"
    want[cube & (image >= 300) & core] = "bone_050"
    want[cube & (image >= 300) & ~core] = "bone_100"
    assert np.array_equal(_names(m), want)
    assert want[7, 4, 5] == "bone_100" and want[6, 4, 5] == "bone_050" and want[5, 3, 4] == "bone_050" and want[5, 2, 4] == "bone_020"
    assert np.array_equal(d, np.array([RHO[n] for n in want.ravel()], np.float32).reshape(shape))
    assert m.dtype == np.uint8 and d.dtype == np.float32


def test_overwrite_order():
    """vessel over lung over body; the air line only inside the body, after fat and before the vessels."""
    shape = (6, 1, 1)
    image = np.array([-950, -950, -950, -950, 20, -950], np.int16).reshape(shape)
    body = np.array([1, 1, 1, 0, 1, 1], np.uint8).reshape(shape)
    lung = np.array([1, 1, 0, 1, 1, 0], np.uint8).reshape(shape)
    vessel = np.array([0, 1, 0, 0, 0, 0], np.uint8).reshape(shape)
    fat = np.array([0, 0, 0, 0, 0, 1], np.uint8).reshape(shape)
    m, _ = _execute(image, body=body, lung=lung, lung_vessel=vessel, fat=fat)
    #  0: lung below -900 inside the body -> air      1: the same voxel in a vessel -> blood       2: body below -900 -> air
    #  3: lung OUTSIDE the body below -900 stays lung 4: lung at 20 HU -> lung                      5: fat below -900 -> air
    assert list(_names(m).ravel()) == ["air", "blood", "air", "lung", "lung", "air"]


def test_skipped_segmentations_and_unmapped_voxels():
    shape = (4, 4, 4)
    image = np.zeros(shape, np.int16)
    body = np.ones(shape, np.uint8)
    liver = np.zeros(shape, np.uint8)
    liver[1:3] = 1
    m, _ = _execute(image, body=body, liver=liver, bone=None, lung=None)   # absent lines are skipped
    assert set(_names(m).ravel()) == {"soft_tissue", "liver"} and np.count_nonzero(m == num("liver")) == 32
    with pytest.raises(ValueError, match=r"^32 voxels are unmapped"):       # no body line: what the liver does not cover is unmapped
        _execute(image, liver=liver)
    with pytest.raises(ValueError, match=r"^64 voxels are unmapped"):
        _execute(image)
    assert np.array_equal(geo.classify_image(image, {"liver": liver}) == geo.UNMAPPED_CLASS, liver == 0)


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_image_types_and_nan(dtype):
    """int16 and float32 images give the same classes at the same values; a NaN fails every comparison: inside a bone it keeps the
    body's class, inside the body it does not become air."""
    shape = (5, 1, 1)
    image = np.array([149, 150, 299, 300, -901], dtype).reshape(shape)
    body = np.ones(shape, np.uint8)
    bone = np.array([1, 1, 1, 1, 0], np.uint8).reshape(shape)
    m, _ = _execute(image, body=body, bone=bone)
    assert list(_names(m).ravel()) == ["red_marrow", "bone_020", "bone_020", "bone_100", "air"]
    if dtype is np.float32:
        image = np.array([149.99, np.nan, 299.99, np.nan, -900.0], dtype).reshape(shape)
        bone = np.array([1, 1, 1, 0, 0], np.uint8).reshape(shape)
        m, _ = _execute(image, body=body, bone=bone)
        assert list(_names(m).ravel()) == ["red_marrow", "soft_tissue", "bone_020", "soft_tissue", "soft_tissue"]
        want = [geo.IMAGE_CLASSES.index(n) for n in ("red_marrow", "soft_tissue", "bone_020", "soft_tissue", "soft_tissue")]
        assert np.array_equal(geo.classify_image(image, {"body": body, "bone": bone}), np.array(want).reshape(shape))


@pytest.mark.parametrize("seed", range(6))
def test_sequential_pipeline_equals_the_closed_form(seed):
    """The mappers applied one after the other (later ones overwriting) against `classify_image`, which decides every voxel from the last
    line down: random masks that touch every border of the volume, random subsets of the segmentations, both image types with NaNs."""
    rng = np.random.default_rng(seed)
    shape = (11, 7, 9)
    table = geo.image_class_table()
    mat_of, rho_of = np.array([t[0] for t in table], np.uint8), np.array([t[1] for t in table], np.float32)
    for trial in range(8):
        image = rng.integers(-1100, 900, size=shape).astype(np.int16 if trial % 2 == 0 else np.float32)
        if image.dtype == np.float32:
            image += rng.random(shape).astype(np.float32)
            image[rng.random(shape) < 0.03] = np.nan
        segs = {"body": (rng.random(shape) < 0.85).astype(np.uint8) * rng.integers(1, 4, size=shape).astype(np.uint8)}
        for name in geo.SEGMENTATION_NAMES[1:]:
            if rng.random() < 0.75:
                segs[name] = (rng.random(shape) < rng.uniform(0.1, 0.9)).astype(np.uint8)
        if "bone" in segs:  # a blob that reaches three faces, so that the erosion's border rule matters
            segs["bone"][:6, :5, 3:] = 1
        cls = geo.classify_image(image, segs)
        m, d = _execute(image, **segs)
        assert cls.max() < 12
        assert np.array_equal(m, mat_of[cls]) and np.array_equal(d, rho_of[cls]), (seed, trial)


def test_outline_commutes_with_the_rot90_between_the_frames():
    """The engine's volume is rot90(k=3) of the geometry arrays in the x/y plane: mapping before or after that rotation is the same."""
    rng = np.random.default_rng(3)
    shape = (9, 6, 5)
    image = rng.integers(-1100, 900, size=shape).astype(np.int16)
    segs = {name: (rng.random(shape) < 0.6).astype(np.uint8) for name in geo.SEGMENTATION_NAMES}
    rot = lambda a: np.rot90(a, k=3, axes=(0, 1))
    assert np.array_equal(rot(geo.classify_image(image, segs)), geo.classify_image(rot(image), {k: rot(v) for k, v in segs.items()}))


def _write_case(tmp_path, image, segs, element_type, spacing=(1.5, 2.0, 2.5)):
    paths = {"image": tmp_path / "ct.mha"}
    recon.write_mha(paths["image"], image.swapaxes(0, 2), spacing, (0.0, 0.0, 0.0), element_type=element_type)
    for name, seg in segs.items():
        paths[name] = tmp_path / f"{name}.mha"
        recon.write_mha(paths[name], seg.swapaxes(0, 2), spacing, (0.0, 0.0, 0.0), element_type="MET_UCHAR")
    return paths


@pytest.mark.parametrize("element_type, dtype", [("MET_SHORT", np.int16), ("MET_FLOAT", np.float32), ("MET_UCHAR", np.uint8)])
def test_from_image_round_trips_through_mha_files(tmp_path, element_type, dtype):
    """`MCGeometry.from_image` on `.mha` files of the three element types equals the pipeline on the arrays; the reader returns the
    element type it read and float files as before."""
    rng = np.random.default_rng(11)
    shape = (10, 8, 6)
    image = rng.integers(0, 250, size=shape).astype(dtype) if dtype is np.uint8 else rng.integers(-1100, 900, size=shape).astype(dtype)
    segs = {"body": np.ones(shape, np.uint8), "bone": (rng.random(shape) < 0.5).astype(np.uint8), "lung": (rng.random(shape) < 0.2).astype(np.uint8),
            "lung_vessel": (rng.random(shape) < 0.05).astype(np.uint8)}
    paths = _write_case(tmp_path, image, segs, element_type)
    back, spacing, origin = recon.read_mha(paths["image"])
    assert back.dtype == dtype and back.shape == shape[::-1] and np.array_equal(back.swapaxes(0, 2), image)
    assert spacing == [1.5, 2.0, 2.5] and origin == [0.0, 0.0, 0.0]
    g = geo.MCGeometry.from_image(paths["image"], body_segmentation_filepath=paths["body"], bone_segmentation_filepath=paths["bone"],
                                  lung_segmentation_filepath=paths["lung"], lung_vessel_segmentation_filepath=paths["lung_vessel"])
    m, d = _execute(image, **segs)
    assert np.array_equal(g.materials, m) and np.array_equal(g.densities, d) and g.image_spacing == (1.5, 2.0, 2.5)
    assert g.image_shape == shape
    # the file's own spacing is fine, another one needs the resampler, a segmenter the network: both say what is missing
    geo.MCGeometry.from_image(paths["image"], body_segmentation_filepath=paths["body"], image_spacing=(1.5, 2.0, 2.5))
    with pytest.raises(NotImplementedError, match=r"utils\.py:76-102"):
        geo.MCGeometry.from_image(paths["image"], body_segmentation_filepath=paths["body"], image_spacing=(1.0, 1.0, 1.0))
    with pytest.raises(NotImplementedError, match="segmentation network"):
        geo.MCGeometry.from_image(paths["image"], segmenter=object(), body_segmentation_filepath=paths["body"])
    with pytest.raises(ValueError, match="unmapped"):
        geo.MCGeometry.from_image(paths["image"], bone_segmentation_filepath=paths["bone"])


def test_float_mha_files_read_as_before(tmp_path):
    v = np.random.default_rng(2).normal(size=(3, 4, 5)).astype(np.float32)
    recon.write_mha(tmp_path / "v.mha", v, (1.0, 2.0, 3.0), (-1.0, -2.0, -3.0))
    assert b"ElementType = MET_FLOAT" in (tmp_path / "v.mha").read_bytes()
    back, spacing, origin = recon.read_mha(tmp_path / "v.mha")
    assert back.dtype == np.float32 and back.tobytes() == v.tobytes() and spacing == [1.0, 2.0, 3.0] and origin == [-1.0, -2.0, -3.0]
    (tmp_path / "bad.mha").write_bytes((tmp_path / "v.mha").read_bytes().replace(b"MET_FLOAT", b"MET_DOUBLE"))
    with pytest.raises(ValueError, match="MET_FLOAT / MET_SHORT / MET_UCHAR"):
        recon.read_mha(tmp_path / "bad.mha")


def test_default_pipeline_has_the_reference_keywords_and_order():
    import inspect
    params = list(inspect.signature(geo.MaterialMapperPipeline.create_default_pipeline).parameters)
    assert params == ["body_segmentation", "bone_segmentation", "muscle_segmentation", "fat_segmentation", "liver_segmentation",
                      "stomach_segmentation", "lung_segmentation", "lung_vessel_segmentation"]
    p = geo.MaterialMapperPipeline.create_default_pipeline(body_segmentation="b")
    assert [type(m).__name__ for m, _ in p] == ["BodyROIMaterialMapper", "BoneMaterialMapper", "LungMaterialMapper", "LiverMaterialMapper",
                                                "StomachMaterialMapper", "MuscleMaterialMapper", "FatMaterialMapper", "AirMaterialMapper",
                                                "LungVesselsMaterialMapper"]
    assert p[0][1] == "b" and p[7][1] == "b" and all(s is None for _, s in p[1:7])
    assert [geo.IMAGE_CLASSES.index(c) for c in ("air", "soft_tissue", "bone_100", "blood")] == [0, 1, 5, 11]
    for name in ("from_image",):
        sig = list(inspect.signature(getattr(geo.MCGeometry, name)).parameters)
        assert sig[:3] == ["image_filepath", "segmenter", "segmenter_kwargs"] and sig[-2:] == ["image_spacing", "engine_context"]
        assert [s for s in sig if s.endswith("_segmentation_filepath")] == [f"{k}_segmentation_filepath" for k in
                                                                           ("body", "bone", "muscle", "fat", "liver", "stomach", "lung", "lung_vessel")]


def test_ctypes_mirrors_match_the_c_layout(engine, tmp_path):
    """sizeof and every field offset of mcgpu_image_class / mcgpu_image_map_report as a C compiler lays them out from the header."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is needed (the oracle is built with one)"
    structs = {"mcgpu_image_class": engine.ImageClass, "mcgpu_image_map_report": engine.ImageMapReport}
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
    assert "#define MCGPU_IMAGE_INT16 0" in header and "#define MCGPU_IMAGE_FLOAT32 1" in header
    assert (engine.IMAGE_INT16, engine.IMAGE_FLOAT32) == (0, 1)


def test_image_entry_points_refuse_a_context_without_device(engine, case_dir):
    """No GPU, no fallback: the mapping's hot path is the HIP kernel; the host statement is `MaterialMapperPipeline.execute`."""
    image = np.zeros((4, 4, 4), np.int16)
    body = np.ones((4, 4, 4), np.uint8)
    with engine.create(case_dir("water"), device=-1) as ctx:
        for call in (lambda: ctx.map_image(image, {"body": body}), lambda: ctx.set_geometry_image(image, {"body": body})):
            with pytest.raises(engine.EngineError) as e:
                call()
            assert e.value.code == -1 and "needs a device" in e.value.message
        with pytest.raises(ValueError, match="unknown segmentations"):
            ctx.map_image(image, {"heart": body})
        with pytest.raises(ValueError, match="shape"):
            ctx.map_image(image, {"body": body[:2]})
