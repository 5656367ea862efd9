"""The breathing signal from the projections alone on the MI355X: the Amsterdam shroud (Zijp, Sonke, van Herk
2004) and the 1-D registration of its consecutive columns, what RTK does with `rtkamsterdamshroud` followed by
`rtkextractshroudsignal`.  RTK is absent here and parity with it is unpinned; what is pinned is the rule in the header of
`csrc/shroud.hip`, its float64 restatement (tests/shroud_ref.py) and the kernels held to that restatement.  There is no CPU fallback.

projections are [n, nv, nu] float32 line integrals as `reconstruction.fdk` and `rooster4d` take them; the shroud is [n, m] float32 (row
r of it belongs to detector row `rows[0] + r`); the signal is [n] float64 in detector rows, x_0 = 0, positive toward larger v.

Caveats.  The amplitude is NOT calibrated: on the test fixture the rule recovers 0.87 x the true amplitude without the unsharp mask
and 1.4 to 2.3 x with it, so the signal is offered for the phase only (`reconstruct_4d(extract_signal=True)`; `reconstruct_4d_mc`,
whose model wants calibrated signals, does not take it).  The default `max_shift` = 16 rows rests on an estimate (about 5 rows per
projection for fast diaphragm motion on the Varian half-fan geometry); it has not been measured on any scan."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

UPLOAD_BATCH = 32  # csrc/shroud.hip: kChunk, the projections that go to the device at a time


class _ShroudOptions(C.Structure):
    """mcgpu_shroud_options (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("n_proj", C.c_int), ("nu", C.c_int), ("nv", C.c_int), ("u_first", C.c_int), ("u_count", C.c_int),
                ("v_first", C.c_int), ("v_count", C.c_int), ("unsharp", C.c_int), ("max_shift", C.c_int), ("device", C.c_int)]


class _ShroudReport(C.Structure):
    """mcgpu_shroud_report (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("reserved", C.c_int), ("ms_upload", C.c_double), ("ms_shroud", C.c_double), ("ms_cost", C.c_double),
                ("ms_total", C.c_double), ("peak_device_bytes", C.c_ulonglong)]


def _library():
    from . import engine
    lib = engine.load_library()
    o, r = C.POINTER(_ShroudOptions), C.POINTER(_ShroudReport)
    for name, argtypes in dict(mcgpu_shroud_extract=[o] + [C.c_void_p] * 4 + [r], mcgpu_shroud_signal=[o] + [C.c_void_p] * 3 + [r],
                               mcgpu_shroud_rows_device=[o] + [C.c_void_p] * 2 + [r]).items():
        getattr(lib, name).argtypes, getattr(lib, name).restype = argtypes, C.c_int
    return engine, lib


def _report_dict(rep: _ShroudReport) -> dict:
    return {name: getattr(rep, name) for name, _ in _ShroudReport._fields_ if name.startswith("ms_") or name == "peak_device_bytes"}


def _range(given: Optional[Sequence[int]], size: int, name: str) -> Tuple[int, int]:
    """(first, count) of `given` = (first, count) or None for everything."""
    if given is None:
        return 0, size
    first, count = (int(v) for v in given)
    if first < 0 or count < 1 or first + count > size:
        raise ValueError(f"{name} = ({first}, {count}): (first, count) inside [0, {size})")
    return first, count


def check_parameters(shape, unsharp, max_shift, rows, columns):
    """The fields n_proj .. max_shift of mcgpu_shroud_options; ValueError for what the library refuses."""
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"projections of shape {tuple(shape)}: a stack [n, nv, nu]")
    n, nv, nu = (int(v) for v in shape)
    u_first, u_count = _range(columns, nu, "columns")
    v_first, v_count = _range(rows, nv, "rows")
    unsharp, max_shift = int(unsharp), int(max_shift)
    if unsharp < 0 or (unsharp and unsharp % 2 == 0):
        raise ValueError(f"unsharp {unsharp}: an odd width, or 0 for no mask")
    if max_shift < 0 or 2 * max_shift >= v_count:
        raise ValueError(f"max_shift {max_shift}: 0 <= 2 max_shift < {v_count} rows is required")
    return n, nu, nv, u_first, u_count, v_first, v_count, unsharp, max_shift


def _extract(projections, unsharp, max_shift, rows, columns, gpu_id, want_shroud, want_costs):
    p = np.ascontiguousarray(projections, dtype=np.float32)
    fields = check_parameters(p.shape, unsharp, max_shift, rows, columns)
    n, m, shifts = fields[0], fields[6], 2 * fields[8] + 1
    engine, lib = _library()
    o = _ShroudOptions(C.sizeof(_ShroudOptions), *fields, int(gpu_id))
    shroud = np.empty((n, m), dtype=np.float32) if want_shroud else None
    costs = np.empty((n - 1, shifts), dtype=np.float64) if want_costs else None
    signal = np.empty(n, dtype=np.float64)
    rep = _ShroudReport(C.sizeof(_ShroudReport))
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    engine._check(lib.mcgpu_shroud_extract(C.byref(o), p.ctypes.data, ptr(shroud), ptr(costs), signal.ctypes.data, C.byref(rep)))
    return shroud, costs, signal, _report_dict(rep)


def amsterdam_shroud(projections, unsharp: int = 17, rows=None, columns=None, gpu_id: int = 0):
    """Stage A -> (shroud float32 [n, m], report dict).  rows / columns: (first, count) of the detector rows that make the shroud and of
    the columns that are summed (None: all); unsharp: odd width of the mask along the projection axis, 0 for none.
    report: ms_upload, ms_shroud, ms_cost, ms_total, peak_device_bytes."""
    shroud, _, _, report = _extract(projections, unsharp, 0, rows, columns, gpu_id, True, False)
    return shroud, report


def shroud_signal(shroud, max_shift: int = 16, gpu_id: int = 0):
    """Stages B and C from a shroud [n, m] on the host -> (signal float64 [n] in rows, not detrended; costs float64
    [n - 1, 2 max_shift + 1]; report dict)."""
    a = np.ascontiguousarray(shroud, dtype=np.float32)
    if a.ndim != 2 or a.size == 0:
        raise ValueError(f"shroud of shape {a.shape}: [n, m]")
    n, m = a.shape
    max_shift = int(max_shift)
    if max_shift < 0 or 2 * max_shift >= m:
        raise ValueError(f"max_shift {max_shift}: 0 <= 2 max_shift < {m} rows is required")
    engine, lib = _library()
    o = _ShroudOptions(C.sizeof(_ShroudOptions), n_proj=n, v_count=m, max_shift=max_shift, device=int(gpu_id))
    costs, signal = np.empty((n - 1, 2 * max_shift + 1), dtype=np.float64), np.empty(n, dtype=np.float64)
    rep = _ShroudReport(C.sizeof(_ShroudReport))
    engine._check(lib.mcgpu_shroud_signal(C.byref(o), a.ctypes.data, costs.ctypes.data, signal.ctypes.data, C.byref(rep)))
    return signal, costs, _report_dict(rep)


def finish_signal(signal, detrend: bool = True, invert: bool = False) -> np.ndarray:
    """What extract_signal does to the cumulative shifts: the least-squares line removed (phase.detrend_linear), then the sign."""
    from . import phase
    x = phase.detrend_linear(signal) if detrend else np.array(signal, dtype=np.float64)
    return -x if invert else x


def extract_signal(projections, unsharp: int = 17, max_shift: int = 16, rows=None, columns=None, detrend: bool = True, invert: bool = False,
                   gpu_id: int = 0) -> np.ndarray:
    """Stages A to C in one call (the shroud never leaves the device) -> signal float64 [n] in detector rows.  detrend: the
    least-squares line is removed (the sum of the shifts drifts); invert: the sign is flipped (positive is toward larger v).
    The amplitude is not calibrated (module docstring): use the signal for the phase."""
    _, _, signal, _ = _extract(projections, unsharp, max_shift, rows, columns, gpu_id, False, False)
    return finish_signal(signal, detrend, invert)
