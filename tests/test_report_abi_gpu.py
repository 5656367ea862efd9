"""Reports of the C ABI that begin with `struct_size` (csrc/hip_host.hpp: check_report, write_report): the library writes
min(the caller's struct_size, sizeof) bytes, hands the caller's struct_size back and refuses one that does not reach past 8 bytes.
Held through raw ctypes for mcgpu_image_map_report, mcgpu_resample_report and mcgpu_register_report, each called with its full size,
cut at a middle field, 16 bytes longer than the library knows it, and 4 bytes long."""
import ctypes as C
import math

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

reg = cases.pkg.registration
SPARE, FILL = 16, 0xA5


def _scalars(rep, name):
    v = getattr(rep, name)
    return list(v) if hasattr(v, "__len__") else [v]


def _hold_the_rule(engine, cls, middle_field, function_name, call):
    """call(pointer to the report) -> return code.  Times are the fields named ms_*; every other field is a count (or, for the mean
    squares of the registration, a fixed function of the inputs) and has to repeat from call to call."""
    lib = engine.load_library()
    size = C.sizeof(cls)

    def run(struct_size):
        buf = (C.c_ubyte * (size + SPARE))(*([FILL] * (size + SPARE)))
        C.c_uint.from_buffer(buf).value = struct_size
        rc = call(C.cast(buf, C.POINTER(cls)))
        return rc, bytes(buf)

    rc, full_bytes = run(size)
    assert rc == 0, lib.mcgpu_last_error()
    full = cls.from_buffer_copy(full_bytes[:size])
    for passed in (size, getattr(cls, middle_field).offset, size + SPARE):
        rc, raw = run(passed)
        assert rc == 0, (passed, lib.mcgpu_last_error())
        cut = min(passed, size)
        assert 8 < cut <= size
        rep = cls.from_buffer_copy(raw[:size])
        assert rep.struct_size == passed
        assert raw[cut:] == bytes([FILL]) * (size + SPARE - cut), passed
        checked = 0
        for name, _ in cls._fields_:
            f = getattr(cls, name)
            if name == "struct_size" or f.offset + f.size > cut:
                continue
            checked += 1
            if name.startswith("ms_"):
                assert all(math.isfinite(v) and v >= 0.0 for v in _scalars(rep, name)), (passed, name)
            else:
                assert _scalars(rep, name) == _scalars(full, name), (passed, name)
        assert checked >= 1 and (passed < size or checked == len(cls._fields_) - 1)
    rc, raw = run(4)
    message = lib.mcgpu_last_error().decode(errors="replace")
    assert rc == -1 and "struct_size" in message and function_name in message, (rc, message)
    assert raw[:4] == (4).to_bytes(4, "little") and raw[4:] == bytes([FILL]) * (size + SPARE - 4)


def test_reports_follow_the_callers_struct_size(engine, case_dir):
    lib = engine.load_library()
    rng = np.random.default_rng(11)
    with engine.create(case_dir("water"), device=0) as ctx:
        # mcgpu_map_image: 6 x 5 x 4 int16, the body segmentation covers it
        image = rng.integers(-1100, 900, size=(4, 5, 6)).astype(np.int16)
        img, ptrs, tab, thr, keep = ctx._image_arguments(image, {"body": np.ones(image.shape, dtype=np.uint8)}, None, None)
        mats, dens = np.empty(img.shape, dtype=np.uint8), np.empty(img.shape, dtype=np.float32)
        n = (C.c_int * 3)(*img.shape[::-1])
        _hold_the_rule(engine, engine.ImageMapReport, "unmapped", "mcgpu_map_image",
                       lambda rep: lib.mcgpu_map_image(ctx.h, n, img.ctypes.data, engine.IMAGE_INT16, ptrs, tab, thr, mats.ctypes.data, dens.ctypes.data, rep))
        full = engine.ImageMapReport(struct_size=C.sizeof(engine.ImageMapReport))
        assert lib.mcgpu_map_image(ctx.h, n, img.ctypes.data, engine.IMAGE_INT16, ptrs, tab, thr, mats.ctypes.data, dens.ctypes.data, C.byref(full)) == 0
        assert sum(full.count) == image.size and full.unmapped == 0 and full.kernel_bytes > 0
        # mcgpu_resample_volume: 5 x 4 x 3 voxels from spacing 2 to 1
        a = rng.normal(size=(5, 4, 3)).astype(np.float32)
        o = engine.ResampleOptions(C.sizeof(engine.ResampleOptions), (C.c_int * 3)(*a.shape), (C.c_double * 3)(2.0, 2.0, 2.0), (C.c_double * 3)(1.0, 1.0, 1.0),
                                   engine.IMAGE_FLOAT32, engine.RESAMPLE_LINEAR, 0.0)
        n_out = (C.c_int * 3)()
        assert lib.mcgpu_resample_plan(C.byref(o), n_out, None, None, None, None, None) == 0
        out = np.empty(tuple(n_out), dtype=np.float32)
        assert out.shape == (10, 8, 6)
        _hold_the_rule(engine, engine.ResampleReport, "ms_download", "mcgpu_resample_volume",
                       lambda rep: lib.mcgpu_resample_volume(ctx.h, C.byref(o), a.ctypes.data, out.ctypes.data, rep))
    # mcgpu_register: 8 x 8 x 8 voxels, one level, one iteration
    _, lib = reg._library()
    fixed, moving = rng.normal(size=(8, 8, 8)).astype(np.float32), rng.normal(size=(8, 8, 8)).astype(np.float32)
    field = np.empty((3, 8, 8, 8), dtype=np.float32)
    ro = reg._options(fixed.shape, 1, 2.25, (1.25, 1.25, 1.25), 1, 0)
    _hold_the_rule(engine, reg._RegisterReport, "ms_resize", "mcgpu_register",
                   lambda rep: lib.mcgpu_register(C.byref(ro), fixed.ctypes.data, moving.ctypes.data, None, field.ctypes.data, rep))
