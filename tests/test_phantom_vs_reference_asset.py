"""Phantom geometries against the reference's bundled assets: the procedural Catphan604 generator reproduces
cbctmc/assets/geometries/catphan604_geometry.pkl.gz voxel for voxel, and the shipped CIRS base geometry
(assets/geometries/base_cirs_geometry.npz) equals base_cirs_geometry.pkl.gz.  The reference's assets are held by their shape,
spacing and the SHA-256 of their voxel arrays (tests/golden/reference_geometry_assets.json, written by
`python tests/test_phantom_vs_reference_asset.py <reference tree>`).  The shipped CIRS asset is pinned by its SHA-256 too, and
the insert builders are checked against independent restatements of geo.py:749-878."""
import hashlib
import gzip
import json
import pickle
import sys
from pathlib import Path

import numpy as np

import cases

ASSETS_PIN = cases.GOLDEN / "reference_geometry_assets.json"
ASSET_FILES = {"catphan604": "cbctmc/assets/geometries/catphan604_geometry.pkl.gz", "base_cirs": "cbctmc/assets/geometries/base_cirs_geometry.pkl.gz"}


class _Stub:
    def __init__(self, *a, **k):
        pass

    def __setstate__(self, state):
        self.__dict__.update(state if isinstance(state, dict) else {})


class _Unpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module.startswith("cbctmc") or module.startswith("ipmi") or module.startswith("vroc"):
            return _Stub
        return super().find_class(module, name)


def voxel_digest(materials, densities, spacing=None):
    """Shape, spacing and SHA-256 of the voxel arrays (materials as uint8, densities as float32, C order)."""
    m = np.asarray(materials)
    m8 = np.ascontiguousarray(m, dtype=np.uint8)
    assert np.array_equal(m8, m), "material numbers beyond uint8"
    return {"shape": list(m.shape), "spacing": None if spacing is None else [float(v) for v in spacing],
            "materials_sha256": hashlib.sha256(m8.tobytes()).hexdigest(),
            "densities_sha256": hashlib.sha256(np.ascontiguousarray(densities, dtype=np.float32).tobytes()).hexdigest()}


def reference_asset(name):
    return json.loads(ASSETS_PIN.read_text())[name]


def test_catphan_generator_matches_bundled_asset():
    ref = reference_asset("catphan604")
    mine = cases.geometry.MCCatPhan604Geometry()
    assert ref["shape"] == [500, 500, 500]
    got = voxel_digest(mine.materials, mine.densities)
    assert got["shape"] == ref["shape"]
    assert got["materials_sha256"] == ref["materials_sha256"]
    assert got["densities_sha256"] == ref["densities_sha256"]


def test_shipped_cirs_base_geometry_equals_bundled_asset():
    ref = reference_asset("base_cirs")
    mine = cases.geometry.MCCIRSPhantomGeometry.from_base_geometry()
    assert mine.image_shape == (305, 300, 152) and list(mine.image_spacing) == ref["spacing"]
    assert voxel_digest(mine.materials, mine.densities, mine.image_spacing) == ref


def test_shipped_cirs_base_geometry_is_pinned():
    g = cases.geometry.MCCIRSPhantomGeometry.from_base_geometry()
    assert hashlib.sha256(g.materials.tobytes()).hexdigest().startswith("c8bf96c16c10209e")
    assert hashlib.sha256(g.densities.tobytes()).hexdigest().startswith("f7b4e8a84a6f1257")
    M = cases.materials
    pairs = {(int(m), round(float(d), 4)) for m, d in zip(*np.unique(np.stack([g.materials.ravel().astype(np.float64), g.densities.ravel()]), axis=1))}
    assert pairs == {(M.material_number("air"), 0.0013), (M.material_number("h2o"), 0.207), (M.material_number("soft_tissue"), 1.0),
                     (M.material_number("red_marrow"), 1.03), (M.material_number("bone_020"), 1.14), (M.material_number("bone_050"), 1.4),
                     (M.material_number("bone_100"), 1.92)}


def test_cirs_inserts_follow_the_reference_recipes():
    """Brute-force restatements on meshgrids (the reference's own formulation, geo.py:749-878) of the masks the
    bounding-box-free broadcasting code in geometry.py builds."""
    G, M = cases.geometry.MCCIRSPhantomGeometry, cases.materials
    shape, c = (60, 50, 48), np.array([31, 24, 20])
    x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    sphere = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= 15.0 ** 2
    assert np.array_equal(G.create_spherical_mask(15.0, shape, c), sphere)
    cz = c[2] + 7.5
    bore = ((x - c[0]) ** 2 + (y - c[1]) ** 2 <= 1.5 ** 2) & (z >= cz - 7.5) & (z <= cz + 7.5)
    want = sphere & ~bore
    assert np.array_equal(G.create_cirs_insert(shape, c), want) and bore.sum() > 0
    base = G.from_base_geometry()
    g = base.place_insert(shift=(0, 0, 5))
    changed = g.materials != base.materials
    assert 13000 < changed.sum() < 14200  # a 30 mm sphere (14137 voxels) minus the bore, minus voxels that already were soft tissue
    assert set(np.unique(g.materials[changed])) == {M.material_number("soft_tissue")}
    zs = np.nonzero(changed.any(axis=(0, 1)))[0]
    assert zs.min() == 71 + 5 - 15 and zs.max() == 71 + 5 + 14  # the upper pole voxel lies in the bore
    lp = base.place_line_pair_insert(gap=4)
    assert lp.image_shape == (1220, 300, 152) and lp.image_spacing == (0.25, 1.0, 1.0)
    al = lp.materials == M.material_number("aluminium")
    assert al.sum() == 4 * 16 * 40 * 40
    xs = np.nonzero(al.any(axis=(1, 2)))[0]
    assert xs.min() == 238 * 4 - 2 * 32 and xs.max() == 238 * 4 - 2 * 32 + 3 * 32 + 15
    lung_eq = (lp.materials == M.material_number("h2o")) & np.isclose(lp.densities, 0.207)
    assert lung_eq[xs.min() + 16: xs.min() + 32, 141, 71].all()
    assert np.array_equal(lp.materials[::4][:222], base.materials[:222])  # untouched in front of the insert


if __name__ == "__main__":  # regenerate the pin: python tests/test_phantom_vs_reference_asset.py <reference tree>
    out = {}
    for name, rel in ASSET_FILES.items():
        with gzip.open(Path(sys.argv[1]) / rel, "rb") as f:
            ref = _Unpickler(f).load()
        spacing = getattr(ref, "image_spacing", None)
        out[name] = voxel_digest(ref.materials, ref.densities, None if spacing is None else tuple(spacing))
    ASSETS_PIN.write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", ASSETS_PIN)
