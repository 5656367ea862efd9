"""Voxelised geometries and the MC-GPU `.vox(.gz)` wire format.

Host-side mirror of the parts of `cbctmc/mc/geometry.py` the engine path needs:
`MCGeometry.save_mcgpu_geometry` / `create_mcgpu_geometry` (geo.py:462-477, :579-623: rot90(k=3) in
the x/y plane and swapped x/y spacing before writing, x fastest), `MCAirGeometry` (geo.py:626-639),
`MCCatPhan604Geometry` (recipe geo.py:902-1068), `pad_to_shape` (geo.py:340-374), `copy` / `warp`
(geo.py:375-439; the warp runs on the GPU through the engine), `MCCIRSPhantomGeometry` (geo.py:642-878:
bundled base geometry + tumour / line-pair inserts), and the CT -> material mapping of `MCGeometry.from_image`
(geo.py:495-577) with its mapper classes and `MaterialMapperPipeline` (geo.py:35-309), written against the rule
stated in DESIGN.md row f8 / csrc/image_map.hpp: segmentations come as arrays, as uncompressed `.mha` files or from the
segmentation network (`segmenter=`: segmentation.MCSegmenter, csrc/segment_net.hip).  The pipeline
here is the host statement of the rule; `engine.Context.map_image` / `set_geometry_image` run it on the GPU.
`resample_image_spacing` (cbctmc/utils.py:76-102: SimpleITK's Resample to another voxel spacing, which `from_image(image_spacing=...)`
applies to the CT and to every segmentation file) runs on the GPU only (`engine.Context.resample_volume`, csrc/resample.hip; the rule:
DESIGN.md row f12 / csrc/resample.hpp); like `MCGeometry.warp` it has no host implementation and needs an `engine_context`.
`MCThoraxLikeGeometry` is NOT a reference class: it is the synthetic patient-like workload of SURVEY.md 8d (input 3)
used by tests and benchmarks.
"""
from __future__ import annotations

import gzip
from pathlib import Path
from typing import Dict, Sequence, Tuple

import numpy as np

from .materials import MATERIALS_125KEV, material_number


class MCGeometry:
    def __init__(self, materials: np.ndarray, densities: np.ndarray,
                 image_spacing: Tuple[float, float, float] = (1.0, 1.0, 1.0)):
        if materials.shape != densities.shape:
            raise ValueError(f"Shape mismatch: {materials.shape=} != {densities.shape=}")
        self.materials = np.ascontiguousarray(materials, dtype=np.uint8)
        self.densities = np.ascontiguousarray(densities, dtype=np.float32)
        self.image_spacing = tuple(float(s) for s in image_spacing)  # mm

    @property
    def image_shape(self) -> Tuple[int, int, int]:
        return self.materials.shape

    @property
    def image_size(self) -> Tuple[float, float, float]:
        return tuple(sh * sp for sh, sp in zip(self.image_shape, self.image_spacing))

    def pad_to_shape(self, target_shape: Sequence[int]) -> "MCGeometry":
        """Centre-pad with air (material 1, density 0.0013) up to `target_shape`."""
        air = MATERIALS_125KEV["air"]
        pads = []
        for have, want in zip(self.image_shape, target_shape):
            extra = max(int(want) - have, 0)
            pads.append((extra // 2, extra - extra // 2))
        mats = np.pad(self.materials, pads, mode="constant", constant_values=material_number("air"))
        dens = np.pad(self.densities, pads, mode="constant", constant_values=np.float32(air))
        return MCGeometry(mats, dens, self.image_spacing)

    def copy(self) -> "MCGeometry":
        g = self.__class__.__new__(self.__class__)
        MCGeometry.__init__(g, self.materials.copy(), self.densities.copy(), self.image_spacing)
        return g

    def warp(self, vector_field: np.ndarray, engine_context) -> "MCGeometry":
        """Nearest-neighbour warp by a dense displacement field [(1,) 3, x, y, z] in voxels, air outside the volume
        (`MCGeometry.warp`, geo.py:386-439: vroc's SpatialTransformer = identity grid + field ->
        `grid_sample(mode="nearest", align_corners=True)`).  Runs on the GPU of `engine_context` (an open
        `engine.Context`); there is no host implementation."""
        field = np.asarray(vector_field, dtype=np.float32)
        if field.ndim == 5:
            field = field[0]
        if field.ndim != 4 or field.shape[0] != 3 or field.shape[1:] != self.image_shape:
            raise ValueError(f"Expected vector_field of shape (3, {self.image_shape}), but got {field.shape=}")
        u = np.ascontiguousarray(np.transpose(field, (0, 3, 2, 1)))  # engine arrays are [z][y][x]; components stay (x, y, z)
        m, d = engine_context.warp_volume(np.transpose(self.materials, (2, 1, 0)), np.transpose(self.densities, (2, 1, 0)), u,
                                          material_number("air"), MATERIALS_125KEV["air"])
        return MCGeometry(np.transpose(m, (2, 1, 0)), np.transpose(d, (2, 1, 0)), self.image_spacing)

    @classmethod
    def from_image(cls, image_filepath, segmenter=None, segmenter_kwargs=None, body_segmentation_filepath=None,
                   bone_segmentation_filepath=None, muscle_segmentation_filepath=None, fat_segmentation_filepath=None,
                   liver_segmentation_filepath=None, stomach_segmentation_filepath=None, lung_segmentation_filepath=None,
                   lung_vessel_segmentation_filepath=None, image_spacing=None, engine_context=None) -> "MCGeometry":
        """A CT image (uncompressed `.mha`, HU) and segmentation files -> geometry (`MCGeometry.from_image`, geo.py:495-577).
        With `engine_context` (an open `engine.Context` with a device) the mapping runs on its GPU (`Context.map_image`), else
        in numpy (`MaterialMapperPipeline.execute`); both give the same arrays.  A `segmenter` (segmentation.MCSegmenter, or any
        object with its `segment`) predicts the segmentations; a given file wins over its prediction.  `segmenter_kwargs` is
        accepted for the reference's signature and not read (the reference does not read it either).  With an `image_spacing` that
        differs from the file's, the image (linear, -1000 outside) and every segmentation file (nearest neighbour, 0 outside) are
        resampled to it on the GPU of `engine_context` (`resample_image_spacing`), a segmenter sees the resampled image and the
        geometry carries `image_spacing`; without `engine_context` that raises NotImplementedError: the resampler has no host
        implementation."""
        image, spacing, segmentations = load_image_and_segmentations(
            image_filepath, segmenter=segmenter, image_spacing=image_spacing, engine_context=engine_context, body=body_segmentation_filepath,
            bone=bone_segmentation_filepath, muscle=muscle_segmentation_filepath, fat=fat_segmentation_filepath,
            liver=liver_segmentation_filepath, stomach=stomach_segmentation_filepath, lung=lung_segmentation_filepath,
            lung_vessel=lung_vessel_segmentation_filepath)
        if engine_context is not None:
            materials, densities = engine_context.map_image(image, segmentations)
        else:
            pipeline = MaterialMapperPipeline.create_default_pipeline(**{f"{k}_segmentation": v for k, v in segmentations.items()})
            materials, densities = pipeline.execute(image)
        return cls(materials, densities, spacing)

    def mcgpu_arrays(self):
        """(materials, densities, spacing_cm) exactly as written to the voxel file (x fastest)."""
        mats = np.rot90(self.materials, k=3, axes=(0, 1))
        dens = np.rot90(self.densities, k=3, axes=(0, 1))
        spacing_cm = (self.image_spacing[1] / 10.0, self.image_spacing[0] / 10.0, self.image_spacing[2] / 10.0)
        return mats, dens, spacing_cm

    def save_mcgpu_geometry(self, filepath, compress: bool = True, engine=None, binary_sidecar: bool = False):
        """Text voxel file of the reference (geo.py:579-623).  `binary_sidecar` (needs `engine`) also writes
        `<stem>.voxbin`, which the engine loads instead of parsing the text."""
        if not (self.densities > 0.0).all():
            raise ValueError("Density can not be zero or negative")
        mats, dens, spacing_cm = self.mcgpu_arrays()
        write_vox(filepath, mats, dens, spacing_cm, compress=compress, engine=engine)
        if binary_sidecar:
            if engine is None:
                raise ValueError("the binary sidecar is written by the engine library")
            nx, ny, nz = mats.shape
            engine.write_voxel_binary(engine.voxel_sidecar_path(filepath), (nx, ny, nz), spacing_cm,
                                      np.transpose(mats, (2, 1, 0)), np.transpose(dens, (2, 1, 0)))


# ---- CT image + segmentations -> (material, density): the rule of DESIGN.md row f8 (csrc/image_map.hpp), on the host
# classes in the order of the engine's 12-entry table; segmentations in the order of its eight pointers
IMAGE_CLASSES = ("air", "soft_tissue", "red_marrow", "bone_020", "bone_050", "bone_100", "lung", "liver", "stomach_intestines",
                 "muscle_tissue", "adipose", "blood")
SEGMENTATION_NAMES = ("body", "bone", "lung", "liver", "stomach", "muscle", "fat", "lung_vessel")
IMAGE_THRESHOLDS = (150.0, 300.0, -900.0)  # red_marrow | bone_020 | bone_050 (HU), and the air line's
UNMAPPED_CLASS = 255


def image_class_table():
    """[(material number, density)] of IMAGE_CLASSES: what the mappers below write and what the engine's table takes."""
    return [(material_number(c), float(MATERIALS_125KEV[c])) for c in IMAGE_CLASSES]


def image_values(image) -> np.ndarray:
    """The image as the rule compares it: int16 stays (every value is exact in float32), anything else becomes float32."""
    a = np.asarray(image)
    return a if a.dtype == np.int16 else a.astype(np.float32, copy=False)


def _inside(segmentation) -> np.ndarray:
    return np.asarray(segmentation) > 0


def bone_outline(mask: np.ndarray) -> np.ndarray:
    """Voxels of `mask` that its erosion by the 6-neighbour cross removes, outside the volume counting as background."""
    from scipy import ndimage
    return mask & ~ndimage.binary_erosion(mask)


def classify_image(image, segmentations: Dict[str, np.ndarray], thresholds=IMAGE_THRESHOLDS) -> np.ndarray:
    """The CLOSED FORM of the rule: index into IMAGE_CLASSES per voxel (UNMAPPED_CLASS where no line applies), decided
    from the last line down instead of by overwriting.  `segmentations`: name of SEGMENTATION_NAMES -> array; missing or
    None = that line is skipped.  `MaterialMapperPipeline.execute` is the sequential statement of the same rule."""
    v = image_values(image).astype(np.float32)
    t0, t1, t2 = (np.float32(t) for t in thresholds)
    s = {k: (_inside(segmentations[k]) if segmentations.get(k) is not None else None) for k in SEGMENTATION_NAMES}
    cls = np.full(v.shape, UNMAPPED_CLASS, dtype=np.uint8)
    todo = np.ones(v.shape, dtype=bool)

    def decide(where, index):
        nonlocal todo
        hit = todo & where
        cls[hit] = index
        todo &= ~hit

    c = IMAGE_CLASSES.index
    if s["lung_vessel"] is not None:
        decide(s["lung_vessel"], c("blood"))
    if s["body"] is not None:
        decide(s["body"] & (v < t2), c("air"))
    for name, ident in (("fat", "adipose"), ("muscle", "muscle_tissue"), ("stomach", "stomach_intestines"), ("liver", "liver"), ("lung", "lung")):
        if s[name] is not None:
            decide(s[name], c(ident))
    if s["bone"] is not None:
        bone = s["bone"]
        decide(bone & (v >= t1) & bone_outline(bone), c("bone_100"))
        decide(bone & (v >= t1), c("bone_050"))
        decide(bone & (t0 <= v) & (v < t1), c("bone_020"))
        decide(bone & (v < t0), c("red_marrow"))
    if s["body"] is not None:
        decide(s["body"], c("soft_tissue"))
        decide(~s["body"], c("air"))
    return cls


class BaseMaterialMapper:
    """One line of the rule: `assignments(image, inside)` -> [(mask, material identifier)], written in that order."""

    def assignments(self, image: np.ndarray, inside: np.ndarray):
        raise NotImplementedError

    def map(self, image, segmentation, materials_output=None, densities_output=None):
        inside = _inside(segmentation)
        materials = np.zeros(inside.shape, dtype=np.uint8) if materials_output is None else materials_output
        densities = np.zeros(inside.shape, dtype=np.float32) if densities_output is None else densities_output
        for mask, ident in self.assignments(image_values(image), inside):
            materials[mask] = material_number(ident)
            densities[mask] = np.float32(MATERIALS_125KEV[ident])
        return materials, densities

    def __repr__(self):
        return f"{self.__class__.__name__}()"


class SingleMaterialMapper(BaseMaterialMapper):
    def __init__(self, target_material: str):
        self.target_material = target_material

    def assignments(self, image, inside):
        return [(inside, self.target_material)]


class BodyROIMaterialMapper(BaseMaterialMapper):
    def assignments(self, image, inside):
        return [(inside, "soft_tissue"), (~inside, "air")]


class BoneMaterialMapper(BaseMaterialMapper):
    def __init__(self, marrow_below=IMAGE_THRESHOLDS[0], dense_from=IMAGE_THRESHOLDS[1]):
        self.marrow_below, self.dense_from = np.float32(marrow_below), np.float32(dense_from)

    def assignments(self, image, inside):
        dense = inside & (image >= self.dense_from)
        return [(inside & (image < self.marrow_below), "red_marrow"),
                (inside & (self.marrow_below <= image) & (image < self.dense_from), "bone_020"),
                (dense, "bone_050"), (dense & bone_outline(inside), "bone_100")]


class AirMaterialMapper(BaseMaterialMapper):
    def __init__(self, below=IMAGE_THRESHOLDS[2]):
        self.below = np.float32(below)

    def assignments(self, image, inside):
        return [(inside & (image < self.below), "air")]


class LungMaterialMapper(SingleMaterialMapper):
    def __init__(self, use_air: bool = False):
        super().__init__("air" if use_air else "lung")


class LungVesselsMaterialMapper(SingleMaterialMapper):
    def __init__(self):
        super().__init__("blood")


class LiverMaterialMapper(SingleMaterialMapper):
    def __init__(self):
        super().__init__("liver")


class StomachMaterialMapper(SingleMaterialMapper):
    def __init__(self):
        super().__init__("stomach_intestines")


class MuscleMaterialMapper(SingleMaterialMapper):
    def __init__(self):
        super().__init__("muscle_tissue")


class FatMaterialMapper(SingleMaterialMapper):
    def __init__(self):
        super().__init__("adipose")


def read_segmentation(path) -> np.ndarray:
    """uint8 [x, y, z] of an uncompressed `.mha` segmentation (file order is x fastest)."""
    from .reconstruction import read_mha
    data, _, _ = read_mha(path)
    return np.ascontiguousarray(np.asarray(data).swapaxes(0, 2), dtype=np.uint8)


class MaterialMapperPipeline(list):
    """[(mapper, segmentation array | file path | None)] executed in order, later entries overwriting earlier ones
    (`MaterialMapperPipeline`, geo.py:237-309).  An entry without segmentation is skipped."""

    def execute(self, image, image_spacing=None):
        """(materials uint8, densities float32) of `image`, in its own layout.  Raises ValueError with the number of voxels
        that no mapper touched (the reference would hand material 0 at density 0 on to the voxel file writer, which refuses it)."""
        if image_spacing is not None:
            raise NotImplementedError("the host pipeline has no resampler: the reference's resample_image_spacing (cbctmc/utils.py:76-102) runs on the "
                                      "GPU here; resample the segmentations first (geometry.resample_image_spacing with engine_context=)")
        materials = densities = None
        for mapper, segmentation in self:
            if segmentation is None:
                continue
            if isinstance(segmentation, (str, Path)):
                segmentation = read_segmentation(segmentation)
            elif not isinstance(segmentation, np.ndarray):
                raise ValueError("a segmentation is an array, a file path or None")
            materials, densities = mapper.map(image, segmentation, materials, densities)
        unmapped = int(np.asarray(image).size) if materials is None else int(np.count_nonzero(materials == 0))
        if unmapped:
            raise ValueError(f"{unmapped} voxels are unmapped: no mapper touches them (a body segmentation is missing)")
        return materials, densities

    @classmethod
    def create_default_pipeline(cls, body_segmentation=None, bone_segmentation=None, muscle_segmentation=None, fat_segmentation=None,
                                liver_segmentation=None, stomach_segmentation=None, lung_segmentation=None, lung_vessel_segmentation=None):
        return cls([(BodyROIMaterialMapper(), body_segmentation), (BoneMaterialMapper(), bone_segmentation),
                    (LungMaterialMapper(use_air=False), lung_segmentation), (LiverMaterialMapper(), liver_segmentation),
                    (StomachMaterialMapper(), stomach_segmentation), (MuscleMaterialMapper(), muscle_segmentation),
                    (FatMaterialMapper(), fat_segmentation), (AirMaterialMapper(), body_segmentation),
                    (LungVesselsMaterialMapper(), lung_vessel_segmentation)])


PREDICTED_LABELS = {"bone": "upper_body_bones", "muscle": "upper_body_muscles", "fat": "upper_body_fat", "liver": "liver", "stomach": "stomach",
                    "lung": "lung", "lung_vessel": "lung_vessels"}  # name of SEGMENTATION_NAMES -> label of segmentation.LABELS; body: not background


def predict_segmentations(image, segmenter) -> dict:
    """{name: uint8 [x, y, z]} of all SEGMENTATION_NAMES from `segmenter.segment(image)` as `from_image` uses it (geo.py:530-542):
    body = (background == 0), the others by their label index.  The prediction comes in the padded shape (every axis at least the
    patch); it is cropped back to the image (left = pad // 2) -- the reference would fail there on the shape mismatch."""
    from .segmentation import get_label_index
    prediction = np.asarray(segmenter.segment(image)[0])
    if callable(getattr(segmenter, "clear_cache", None)):
        segmenter.clear_cache()
    if prediction.ndim != 4 or any(have < want for have, want in zip(prediction.shape[1:], image.shape)):
        raise ValueError(f"the segmenter returned shape {prediction.shape} for an image of shape {image.shape}")
    crop = tuple(slice((have - want) // 2, (have - want) // 2 + want) for have, want in zip(prediction.shape[1:], image.shape))
    out = {"body": prediction[get_label_index("background")][crop] == 0}
    for name, label in PREDICTED_LABELS.items():
        out[name] = prediction[get_label_index(label)][crop]
    return {name: np.ascontiguousarray(seg, dtype=np.uint8) for name, seg in out.items()}


IMAGE_DEFAULT_HU = -1000.0  # of resampled CT voxels outside the file's volume (geo.py:514-519); segmentations get 0 (geo.py:252-261)


def spacing_differs(image_spacing, spacing) -> bool:
    """Whether a requested `image_spacing` (None: none requested) asks for another grid than the file's `spacing`."""
    return image_spacing is not None and not np.allclose(np.asarray(image_spacing, dtype=np.float64), spacing, rtol=0.0, atol=1e-9)


def resample_image_spacing(image, spacing, new_spacing, resampler="linear", default_voxel_value=0.0, engine_context=None) -> np.ndarray:
    """`image` (3-D array; uint8, int16 or float32) at `spacing` -> the same element type at `new_spacing`, one spacing per array axis
    (`resample_image_spacing`, cbctmc/utils.py:76-102, on arrays instead of SimpleITK images; `resampler`: "linear" or "nearest").
    `new_spacing=None` returns the input.  Runs on the GPU of `engine_context` (an open `engine.Context` with a device); there is no
    host implementation.  The rule, and what of it is not pinned against SimpleITK: DESIGN.md row f12 / csrc/resample.hpp."""
    if new_spacing is None:
        return image
    if engine_context is None:
        raise NotImplementedError("the resampler (the reference's resample_image_spacing, cbctmc/utils.py:76-102) runs on the GPU and has no host "
                                  "implementation: pass engine_context= (an open engine.Context with a device)")
    return engine_context.resample_volume(image, spacing, new_spacing, interpolator=resampler, default_value=default_voxel_value)


def load_image_and_segmentations(image_filepath, segmenter=None, image_spacing=None, engine_context=None, **segmentation_filepaths):
    """(image [x, y, z], spacing mm, {name: uint8 [x, y, z]}) of `.mha` files, as `from_image` takes them.  Keywords: the names of
    SEGMENTATION_NAMES -> file path or None.  A `segmenter` (an object with a callable `segment`, such as
    `segmentation.MCSegmenter`) predicts all eight; a given file wins over its prediction.  With an `image_spacing` other than the
    file's, the image (linear, -1000 outside) and every segmentation file (nearest neighbour, 0 outside) are resampled to it on the GPU
    of `engine_context` -- the segmenter sees the resampled image -- and the returned spacing is `image_spacing`."""
    from .reconstruction import read_mha
    if segmenter is not None and not callable(getattr(segmenter, "segment", None)):
        raise NotImplementedError("the segmentation network is given as an object with a `segment(image)` method "
                                  "(segmentation.MCSegmenter); anything else is not understood: pass that, or the segmentations as files")
    data, spacing, _ = read_mha(image_filepath)
    if data.ndim != 3:
        raise ValueError(f"{image_filepath}: a 3-D image is needed")
    spacing = tuple(float(v) for v in spacing)
    resample_to = tuple(float(v) for v in image_spacing) if spacing_differs(image_spacing, spacing) else None
    if resample_to is not None and engine_context is None:
        raise NotImplementedError(f"resampling from spacing {spacing} to {resample_to} (the reference's resample_image_spacing, "
                                  "cbctmc/utils.py:76-102) runs on the GPU and has no host implementation: pass engine_context= "
                                  "(an open engine.Context with a device), or resample the files first")
    image = np.ascontiguousarray(np.asarray(data).swapaxes(0, 2))
    image = resample_image_spacing(image, spacing, resample_to, "linear", IMAGE_DEFAULT_HU, engine_context)
    unknown = set(segmentation_filepaths) - set(SEGMENTATION_NAMES)
    if unknown:
        raise TypeError(f"unknown segmentations {sorted(unknown)}")
    segmentations = predict_segmentations(image, segmenter) if segmenter is not None else {}
    for name in SEGMENTATION_NAMES:
        path = segmentation_filepaths.get(name)
        if path is None:
            continue
        seg = resample_image_spacing(read_segmentation(path), spacing, resample_to, "nearest", 0.0, engine_context)
        if seg.shape != image.shape:
            raise ValueError(f"{path}: shape {seg.shape} differs from the image's {image.shape}")
        segmentations[name] = seg
    return image, spacing if resample_to is None else resample_to, segmentations


def write_vox(filepath, materials_xyz: np.ndarray, densities_xyz: np.ndarray, spacing_cm, compress=True, engine=None):
    """Write a voxel file; arrays are indexed [x, y, z]; the file runs x fastest, then y, then z.

    With `engine` (the loaded C-ABI library wrapper) the multi-threaded C++ writer is used;
    otherwise a pure-Python writer (fine for the small test volumes).  Body format as
    `cbctmc/mc/voxel_data.pyx:12-31`: "<mat> <density:.6f>", blank line after each x-row and
    another after each slice.
    """
    filepath = str(filepath)
    nx, ny, nz = materials_xyz.shape
    m_lin = np.ascontiguousarray(np.transpose(materials_xyz, (2, 1, 0)), dtype=np.uint8)   # [z][y][x]
    d_lin = np.ascontiguousarray(np.transpose(densities_xyz, (2, 1, 0)), dtype=np.float32)
    if engine is not None:
        engine.write_voxel_file(filepath, (nx, ny, nz), spacing_cm, m_lin, d_lin, gzip=compress)
        return
    head = (
        "[SECTION VOXELS HEADER v.2008-04-13]\n"
        f"{nx} {ny} {nz}  # SIZE IN X, Y, Z\n"
        f"{spacing_cm[0]} {spacing_cm[1]} {spacing_cm[2]}  # VOXEL SPACING IN X, Y, Z\n"
        "1  # COLUMN NUMBER WHERE MATERIAL ID IS LOCATED\n2  # COLUMN NUMBER WHERE MASS DENSITY IS LOCATED\n"
        "1  # BLANK LINES AT END OF X,Y-CYCLES (1=YES, 0=NO)\n[END OF VXH SECTION]\n#\n"
    )
    parts = [head]
    for k in range(nz):
        for j in range(ny):
            row_m, row_d = m_lin[k, j], d_lin[k, j]
            parts.append("".join(f"{int(a)} {float(b):.6f}\n" for a, b in zip(row_m, row_d)))
            parts.append("\n")
        parts.append("\n")
    text = "".join(parts)
    if compress:
        with gzip.open(filepath, "wt", compresslevel=1) as f:
            f.write(text)
    else:
        with open(filepath, "wt") as f:
            f.write(text)


class MCAirGeometry(MCGeometry):
    """One 2000 mm voxel of air: the flat-field ("air") scan geometry (geo.py:626-639)."""

    def __init__(self, image_spacing=(2000.0, 2000.0, 2000.0)):
        super().__init__(np.full((1, 1, 1), material_number("air"), dtype=np.uint8),
                         np.full((1, 1, 1), MATERIALS_125KEV["air"], dtype=np.float32), image_spacing)


def _cylinder(shape, center, radius, height):
    """Boolean [x,y,z] mask: (x-cx)^2+(y-cy)^2 <= r^2 and cz-h/2 <= z < cz+h/2 on voxel indices."""
    x = np.arange(shape[0], dtype=np.float64)[:, None]
    y = np.arange(shape[1], dtype=np.float64)[None, :]
    disk = (x - center[0]) ** 2 + (y - center[1]) ** 2 <= radius ** 2
    z = np.arange(shape[2], dtype=np.float64)
    zsel = (z >= center[2] - height / 2) & (z < center[2] + height / 2)
    return disk, zsel


class MCCatPhan604Geometry(MCGeometry):
    """Catphan 604 sensitometry module in a water-filled body (recipe: geo.py:902-1068).

    angle [deg], distance/radius/length [voxels at 1 mm].  Later entries overwrite earlier ones.
    """

    BODY = [("h2o", 0.0, 0.0, 100.0, 100.0)]
    SENSITOMETRY = [
        ("air", 90, 58.7, 6.5, 24.0), ("teflon", 60, 58.7, 6.5, 24.0), ("delrin", 0, 58.7, 6.5, 24.0),
        ("bone_020", 330, 58.7, 6.5, 24.0), ("acrylic", 300, 58.7, 6.5, 24.0), ("air", 270, 58.7, 6.5, 24.0),
        ("polystyrene", 240, 58.7, 6.5, 24.0), ("ldpe", 180, 58.7, 6.5, 24.0), ("bone_050", 150, 58.7, 6.5, 24.0),
        ("pmp", 120, 58.7, 6.5, 24.0), ("h2o", 0, 0.0, 30.0, 40.0),
    ]
    CIRCULAR_SYMMETRY = [("air", 135, 35.355, 1.5, 24.0), ("air", 45, 35.355, 1.5, 24.0),
                         ("air", 315, 35.355, 1.5, 24.0), ("air", 225, 35.355, 1.5, 24.0)]

    def __init__(self, shape=(500, 500, 500), image_spacing=(1.0, 1.0, 1.0), scale: float = 1.0,
                 material_numbers: Dict[str, int] | None = None):
        """`scale` shrinks all lengths (voxel units) for reduced test phantoms; `material_numbers`
        overrides the MC-GPU material numbering (default: the reference's 22-material order)."""
        num = material_numbers or {k: material_number(k) for k in MATERIALS_125KEV}
        center = np.array(shape, dtype=np.float64) / 2
        mats = np.full(shape, num["air"], dtype=np.uint8)
        dens = np.full(shape, MATERIALS_125KEV["air"], dtype=np.float32)
        for group in (self.BODY, self.SENSITOMETRY, self.CIRCULAR_SYMMETRY):
            for ident, angle, distance, radius, length in group:
                phi = angle * np.pi / 180.0
                c = np.array([np.cos(phi), -np.sin(phi), 0.0]) * (distance * scale) + center
                disk, zsel = _cylinder(shape, c, radius * scale, length * scale)
                xs, ys = np.nonzero(disk)
                zs = np.nonzero(zsel)[0]
                if xs.size == 0 or zs.size == 0:
                    continue
                mats[xs[:, None], ys[:, None], zs[None, :]] = num[ident]
                dens[xs[:, None], ys[:, None], zs[None, :]] = np.float32(MATERIALS_125KEV[ident])
        super().__init__(mats, dens, image_spacing)


class MCWaterPhantomGeometry(MCGeometry):
    """Water cylinder in air: the phantom of the water pre-correction fit (geo.py:1106-1165; scripts/fit_wpc.py).  Radius 100 mm and
    length 150 mm along z unless given, centred at shape / 2 (voxel indices, as the reference centres it); isotropic spacing only."""

    RADIUS, LENGTH = 100.0, 150.0  # mm

    def __init__(self, shape=(500, 500, 500), image_spacing=(1.0, 1.0, 1.0), radius: float | None = None, length: float | None = None):
        if len(set(image_spacing)) > 1:
            raise ValueError("Image spacing must be isotropic")
        s = float(image_spacing[0])
        center = np.array(shape, dtype=np.float64) / 2
        mats = np.full(shape, material_number("air"), dtype=np.uint8)
        dens = np.full(shape, MATERIALS_125KEV["air"], dtype=np.float32)
        disk, zsel = _cylinder(shape, center, (radius or self.RADIUS) / s, (length or self.LENGTH) / s)
        body = disk[:, :, None] & zsel[None, None, :]
        mats[body] = material_number("h2o")
        dens[body] = np.float32(MATERIALS_125KEV["h2o"])
        super().__init__(mats, dens, image_spacing)


class MCBoxGeometry(MCGeometry):
    """Uniform block of one material (test geometry)."""

    def __init__(self, shape=(32, 32, 32), image_spacing=(5.0, 5.0, 5.0), material="h2o", density=None, number=None):
        n = number if number is not None else material_number(material)
        rho = MATERIALS_125KEV[material] if density is None else density
        super().__init__(np.full(shape, n, dtype=np.uint8), np.full(shape, rho, dtype=np.float32), image_spacing)


ASSETS = Path(__file__).resolve().parent / "assets"


class MCCIRSPhantomGeometry(MCGeometry):
    """CIRS dynamic thorax phantom (geo.py:642-878).  The base geometry is the reference's bundled segmented CT
    (305 x 300 x 152 voxels of 1 mm; air, lung-equivalent = h2o at 0.207, soft_tissue, red_marrow, bone_020/050/100),
    shipped here as `assets/geometries/base_cirs_geometry.npz` (same arrays, see oracle/gen_cirs_asset.py)."""

    @classmethod
    def from_base_geometry(cls) -> "MCCIRSPhantomGeometry":
        with np.load(ASSETS / "geometries" / "base_cirs_geometry.npz") as f:
            return cls(f["materials"], f["densities"], tuple(float(s) for s in f["image_spacing"]))

    @staticmethod
    def create_spherical_mask(radius: float, shape, sphere_center) -> np.ndarray:
        """Voxels with (x-cx)^2 + (y-cy)^2 + (z-cz)^2 <= r^2 on integer voxel indices (geo.py:749-761)."""
        x, y, z = (np.arange(n, dtype=np.float64) for n in shape)
        return ((x[:, None, None] - sphere_center[0]) ** 2 + (y[None, :, None] - sphere_center[1]) ** 2
                + (z[None, None, :] - sphere_center[2]) ** 2) <= radius ** 2

    @staticmethod
    def create_cirs_insert(shape, insert_center) -> np.ndarray:
        """The 30 mm tumour sphere with its 3 mm marker bore: a cylinder of radius 1.5 from the sphere centre to its
        upper pole (both ends inclusive) is cut out (geo.py:763-792)."""
        radius = 15.0
        c = np.asarray(insert_center, dtype=np.float64)
        mask = MCCIRSPhantomGeometry.create_spherical_mask(radius, shape, c)
        x, y, z = (np.arange(n, dtype=np.float64) for n in shape)
        zc = c[2] + radius / 2
        bore = (((x[:, None, None] - c[0]) ** 2 + (y[None, :, None] - c[1]) ** 2 <= 1.5 ** 2)
                & (z[None, None, :] >= zc - radius / 2) & (z[None, None, :] <= zc + radius / 2))
        mask[bore] = False
        return mask

    def place_insert(self, shift=(0, 0, 0), insert_center=(238, 141, 71)) -> "MCCIRSPhantomGeometry":
        """Soft-tissue tumour insert at `insert_center + shift` [voxels] (geo.py:865-878)."""
        mask = self.create_cirs_insert(self.image_shape, np.asarray(insert_center) + np.asarray(shift))
        g = self.copy()
        g.materials[mask] = material_number("soft_tissue")
        g.densities[mask] = np.float32(MATERIALS_125KEV["soft_tissue"])
        return g

    def place_line_pair_insert(self, gap: float = 4) -> "MCCIRSPhantomGeometry":
        """Resolution insert: the x axis is refined 4x (0.25 mm voxels), then 4 line pairs of aluminium / lung-equivalent
        slabs, each `gap` mm wide and 40 x 40 voxels across, are written ending at x = 238 mm (geo.py:794-863)."""
        g = self.copy()
        g.materials = np.repeat(g.materials, 4, axis=0)
        g.densities = np.repeat(g.densities, 4, axis=0)
        g.image_spacing = (0.25, 1.0, 1.0)
        gap_voxel = int(gap // g.image_spacing[0])
        pair = 2 * gap_voxel
        n_pairs, width = 4, 20
        cx = int(238 / g.image_spacing[0] - n_pairs / 2 * pair)
        cy, cz = int(141 / g.image_spacing[1]), int(71 / g.image_spacing[2])
        ys, zs = slice(cy - width, cy + width), slice(cz - width, cz + width)
        for i in range(n_pairs):
            a = cx + i * pair
            g.materials[a:a + gap_voxel, ys, zs] = material_number("aluminium")
            g.densities[a:a + gap_voxel, ys, zs] = np.float32(MATERIALS_125KEV["aluminium"])
            g.materials[a + gap_voxel:a + pair, ys, zs] = material_number("h2o")
            g.densities[a + gap_voxel:a + pair, ys, zs] = np.float32(0.207 * MATERIALS_125KEV["h2o"])
        return g

    def downsample(self, step: int) -> "MCCIRSPhantomGeometry":
        """Every `step`-th voxel at `step` times the spacing (reduced test phantoms; not a reference method)."""
        g = self.__class__.__new__(self.__class__)
        MCGeometry.__init__(g, self.materials[::step, ::step, ::step], self.densities[::step, ::step, ::step],
                            tuple(s * step for s in self.image_spacing))
        return g


class MCThoraxLikeGeometry(MCGeometry):
    """Synthetic patient-like thorax (input 3; BASELINE config 4 shape 512 x 512 x 256 at 1 mm): seeded
    ellipsoids carrying the tissue classes of the reference's material mapper at their NOMINAL densities (the reference
    maps every class to its nominal density, geo.py:72-74).  Body soft tissue with an adipose rim and a muscle layer,
    two lungs with vessels (blood), heart (blood + muscle wall), liver, stomach, spine (bone_100 shell, red_marrow core,
    cartilage discs), ribs (bone_050), sternum (bone_020), glands, and `n_nodules` seeded soft-tissue nodules in the
    lungs.  Lengths scale with the shape, so reduced shapes give the same anatomy at coarser voxels.

    `bone_texture=True` gives the bones the voxel-level texture the reference's `BoneMaterialMapper` produces on a real CT
    (geo.py:138-166): inside the bone segmentation every voxel is classed by its own HU value -- red_marrow below 150, bone_020
    up to 300, bone_050 above, bone_100 for the one-voxel outline above 300 -- here from a seeded, smoothed random HU field
    around each structure's nominal value, so neighbouring voxels of a rib or a vertebra differ in material.  The same switch applies
    the reference's `AirMaterialMapper` (geo.py:168-183: voxels below -900 HU become air) to a seeded HU field of the lungs around
    -820 HU: one lung voxel in eight is air, scattered through the parenchyma as on a real CT."""

    def __init__(self, shape=(512, 512, 256), image_spacing=(1.0, 1.0, 1.0), seed: int = 1234, n_nodules: int = 24, bone_texture: bool = False):
        rng = np.random.default_rng(seed)
        scale = [n / r for n, r in zip(shape, (512.0, 512.0, 256.0))]
        # coordinates in "1 mm voxels of the full-size phantom", origin at the volume centre
        ax = [(np.arange(n, dtype=np.float32) + np.float32(0.5) - np.float32(n / 2)) / np.float32(sc) for n, sc in zip(shape, scale)]
        mats = np.full(shape, material_number("air"), dtype=np.uint8)
        dens = np.full(shape, MATERIALS_125KEV["air"], dtype=np.float32)

        def ell(c, a, cut=None):
            """(slices, mask) of the ellipsoid centre c, half axes a, inside its bounding box."""
            sl = []
            for k in range(3):
                lo, hi = np.searchsorted(ax[k], c[k] - a[k], "left"), np.searchsorted(ax[k], c[k] + a[k], "right")
                sl.append(slice(int(lo), int(hi)))
            x, y, z = ax[0][sl[0]][:, None, None], ax[1][sl[1]][None, :, None], ax[2][sl[2]][None, None, :]
            m = ((x - c[0]) / a[0]) ** 2 + ((y - c[1]) / a[1]) ** 2 + ((z - c[2]) / a[2]) ** 2 <= 1.0
            if cut is not None:
                m = m & cut(x, y, z)
            return tuple(sl), m

        def put(c, a, ident, only=None, cut=None):
            """Fill the ellipsoid with `ident`; `only` restricts it to voxels currently holding that material."""
            sl, m = ell(c, a, cut)
            if only is not None:
                m = m & (mats[sl] == material_number(only))
            mats[sl][m] = material_number(ident)
            dens[sl][m] = np.float32(MATERIALS_125KEV[ident])

        BX, BY, INF = 225.0, 165.0, 1.0e4
        put((0, 0, 0), (BX, BY, INF), "adipose")
        put((0, 0, 0), (BX - 14, BY - 13, INF), "muscle_tissue")
        put((0, 0, 0), (BX - 27, BY - 25, INF), "soft_tissue")
        for k in range(-6, 7):  # ribs: thin elliptical shells in the soft tissue, interrupted at the front
            put((0, 0, k * 20.0), (BX - 29, BY - 27, 4.5), "bone_050", only="soft_tissue", cut=lambda x, y, z: y > -95)
            put((0, 0, k * 20.0), (BX - 40, BY - 37, 4.5), "soft_tissue", only="bone_050")
        for s in (-1, 1):
            put((s * 92, -10, 10), (74, 102, 115), "lung")
            for k in range(9):  # vessels
                c = (s * (92 + rng.uniform(-38, 38)), -10 + rng.uniform(-60, 60), 10 + rng.uniform(-80, 80))
                put(c, (rng.uniform(3, 6), rng.uniform(3, 6), rng.uniform(25, 60)), "blood", only="lung")
            for k in range(n_nodules // 2):
                c = (s * (92 + rng.uniform(-45, 45)), -10 + rng.uniform(-70, 70), 10 + rng.uniform(-90, 90))
                r = rng.uniform(4, 11)
                put(c, (r, r, r), "soft_tissue", only="lung")
        put((15, -36, 18), (54, 47, 48), "muscle_tissue")   # heart wall
        put((15, -36, 18), (43, 36, 39), "blood")           # chambers
        put((-70, -6, -95), (90, 80, 40), "liver", only="soft_tissue")
        put((78, -20, -98), (54, 47, 30), "stomach_intestines", only="soft_tissue")
        put((0, 105, 0), (26, 26, INF), "bone_100")         # vertebral column
        put((0, 105, 0), (17, 17, INF), "red_marrow")
        for k in range(-6, 7):
            put((0, 105, k * 20.0 + 10.0), (26, 26, 2.5), "cartilage")
        put((0, -128, 20), (26, 8, 70), "bone_020")         # sternum
        for s in (-1, 1):
            put((s * 122, -80, 60), (20, 13, 22), "glands_others", only="soft_tissue")
        if bone_texture:
            from scipy import ndimage
            nominal_hu = {"red_marrow": 90.0, "bone_020": 230.0, "bone_050": 420.0, "bone_100": 700.0}
            bone = np.zeros(shape, dtype=bool)
            hu = np.zeros(shape, dtype=np.float32)
            for ident, value in nominal_hu.items():
                m = mats == material_number(ident)
                bone |= m
                hu[m] = value
            sl = tuple(slice(int(lo), int(hi) + 1) for lo, hi in ((i.min(), i.max()) for i in np.nonzero(bone)))  # the bones' bounding box
            noise = ndimage.gaussian_filter(np.random.default_rng(seed + 1).standard_normal(hu[sl].shape).astype(np.float32), 0.8)
            hu_b = hu[sl] + np.float32(170.0 / float(noise.std())) * noise
            mask = bone[sl]
            outline = mask & ~ndimage.binary_erosion(mask)
            for ident, m in (("red_marrow", mask & (hu_b < 150)), ("bone_020", mask & (hu_b >= 150) & (hu_b < 300)),
                             ("bone_050", mask & (hu_b >= 300)), ("bone_100", outline & (hu_b >= 300))):
                mats[sl][m] = material_number(ident)
                dens[sl][m] = np.float32(MATERIALS_125KEV[ident])
            lung = mats == material_number("lung")
            sl = tuple(slice(int(i.min()), int(i.max()) + 1) for i in np.nonzero(lung))
            noise = ndimage.gaussian_filter(np.random.default_rng(seed + 2).standard_normal(mats[sl].shape).astype(np.float32), 1.0)
            air = lung[sl] & (np.float32(-820.0) + np.float32(70.0 / float(noise.std())) * noise < np.float32(-900.0))
            mats[sl][air] = material_number("air")
            dens[sl][air] = np.float32(MATERIALS_125KEV["air"])
        super().__init__(mats, dens, image_spacing)
