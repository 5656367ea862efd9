"""SHA-256 of what the reconstruction entry points return on the tests' small cases, as one JSON object: run it once per library
(MCGPU_AMD_LIB) in one session on one box and compare the two objects key for key -- hipFFT is in the FDK path, so digests are
comparable only within one installation.  The cases are the tests' own builders (tests/ goes on the path):
  fdk      reconstruction.fdk on test_fdk_configs.case for views_1, views_3, varying_offsets, explicit_origin and pad_flip_-11.64_1,
           hipFFT and direct ramp; the water pre-correction (0, 1.05, 0.01) on varying_offsets
  wpc_fit  water_precorrection.normal_equations on wpc_ref.problem("half_fan"), slabs (0, 1), (27, 3), (0, 30), orders 1 and 7, both
           channel layouts, both ramps; "wide" at order 2
  rooster  rooster4d_stage "back" and "forward" on every test_rooster4d_configs.CONFIGS, and one rooster4d call at `odd` with a
           water pre-correction
  fp       project_forward on the thin_* and deg45 cases of test_forward_projection_configs
  fdk_motion      reconstruction.fdk_motion on every entry of test_fdk_motion.CASES
  rooster_motion  rooster4d_motion_stage "warp", "unwarp" and "tv_time_motion" (5 iterations, gamma 0.05, the negated model back) on
                  test_rooster4d_motion's 13 x 5 x 7 small case at K = 1, 2, 3 and 4, and one rooster4d_motion call on the case of
                  test_rooster4d_motion_equals_the_restated_loop_and_repeats_bit_for_bit (volume and residuals)
  register        registration.register on test_registration_gpu's whole-loop case and its (41, 40, 41) case: field, msd_before, msd_after
  invert          registration.invert_field (initial v_0, 5 steps) on test_field_inverse_gpu._fields at (17, 13, 11) and (41, 40, 41):
                  the inverse and the four norms; composition_residual on the same: r and its two norms
--one-slice adds, on "half_fan" with the direct ramp at order 1, slabs (0, 1) and (29, 1), both layouts: the number of float32 words
in which basis_mean[n] of the fused call differs from fdk(..., water_pre_correction=e_n)[0][:, y, :] (tests/test_wpc_fit_gpu.py).
Usage: [MCGPU_AMD_LIB=other.so] python tools/recon_digest.py [--one-slice] [--out FILE.json]"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
from __graft_entry__ import load_package  # noqa: E402

WPC = (0.0, 1.05, 0.01)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def ramp(direct):
    if direct:
        os.environ["MCGPU_FDK_DIRECT_RAMP"] = "1"
    else:
        os.environ.pop("MCGPU_FDK_DIRECT_RAMP", None)
    return "direct" if direct else "fft"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one-slice", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = load_package()
    pkg.engine.load_library()
    recon, wp = pkg.reconstruction, pkg.water_precorrection
    import test_fdk_configs as F
    import test_field_inverse_gpu as FI
    import test_fdk_motion as FM
    import test_forward_projection_configs as J
    import test_registration_gpu as RG
    import test_rooster4d_motion as RM
    import test_rooster4d_configs as R
    import wpc_ref as W
    out = {}

    for direct in (False, True):
        route = ramp(direct)
        for name in ("views_1", "views_3", "varying_offsets", "explicit_origin", "pad_flip_-11.64_1"):
            c = F.case(name)
            out[f"fdk {name} {route}"] = sha(c.hip(c.projections()))
        c = F.case("varying_offsets")
        out[f"fdk varying_offsets wpc {route}"] = sha(c.hip(c.projections(), WPC))
        for name, slabs, orders in (("half_fan", ((0, 1), (27, 3), (0, 30)), (1, 7)), ("wide", ((0, 1),), (2,))):
            p = W.problem(name)
            for slab in slabs:
                for order in orders:
                    for layout in (1, 2):
                        B, a, basis, _ = wp.normal_equations(*p.fdk_args(), p.weight, p.template, slab, order, p.origin, p.hann, p.hann_y, p.pad,
                                                             channel_layout=layout)
                        out[f"wpc_fit {name} slab {slab} order {order} layout {layout} {route}"] = sha(B, a, basis)
    ramp(False)

    for name in R.CONFIGS:
        cfg = R.config(name)
        q = cfg.stage("forward", cfg.field(5))
        out[f"rooster {name} forward"] = sha(q)
        out[f"rooster {name} back"] = sha(cfg.stage("back", q))
    cfg = R.config("odd")
    vol, rep = cfg.rooster4d(cfg.stage("forward", cfg.field(17)), niter=2, cgiter=3, tviter=5, gamma_space=0.002, gamma_time=0.002, positivity=False,
                             water_pre_correction=WPC)
    out["rooster odd whole call wpc"] = sha(vol, rep["residuals"])

    for name in ["thin_%d_%d_%d" % s for s in J.THIN_SHAPES] + ["deg45"]:
        out[f"fp {name}"] = sha(J.case(name).hip())

    for name in FM.CASES:
        out[f"fdk_motion {name}"] = sha(FM._fdk_motion(name)[0])

    for K in (1, 2, 3, 4):
        x, mean, coef, states = RM._small_case(K)[:4]
        model, back, zero = (recon.MotionModel(f * mean, f * coef, np.zeros(K), spacing=RM.SMALL_SPACING) for f in (1.0, -1.0, 0.0))
        for stage, pair, kw in (("warp", (model, zero), {}), ("unwarp", (zero, model), {}), ("tv_time_motion", (model, back), dict(tviter=5, gamma_time=0.05))):
            out[f"rooster_motion small K {K} {stage}"] = sha(recon.rooster4d_motion_stage(stage, x, *pair, states, RM.SMALL_DIM, RM.SMALL_SPACING, **kw)[0])
    geo, ph = RM.base._geometry(), RM.base._phase()
    vol, rep = recon.rooster4d_motion(RM.base._projections(geo, ph), geo, (RM.PIX, RM.PIX), None, ph, *RM._motion_models(RM._k2_models()), RM._signals(ph), RM.DIM,
                                      RM.SPACING, frames=RM.FRAMES, niter=2, cgiter=3, tviter=5, gamma_space=0.002, gamma_time=0.002)
    out["rooster_motion whole call"] = sha(vol, rep["residuals"])

    reg = pkg.registration
    for name, (fixed, moving, kw) in (("whole loop", RG._whole_loop_case()), ("41x40x41", RG._sum_order_case())):
        u, rep = reg.register(fixed, moving, **kw)
        out[f"register {name}"] = sha(u, np.float64(rep["msd_before"]), np.float64(rep["msd_after"]))
    for shape in ((17, 13, 11), (41, 40, 41)):
        u, v0 = FI._fields(shape)
        v, rep = reg.invert_field(u, iterations=5, initial=v0)
        out[f"invert {FI.ids(shape)}"] = sha(v, np.float64([rep[k] for k in ("residual_max_before", "residual_rms_before", "residual_max_after", "residual_rms_after")]))
        r, rep = reg.composition_residual(u, v0)
        out[f"invert {FI.ids(shape)} residual"] = sha(r, np.float64([rep["residual_max"], rep["residual_rms"]]))

    if args.one_slice:
        ramp(True)
        p = W.problem("half_fan")
        for y in (0, 29):
            single = [recon.fdk(*p.fdk_args(), p.origin, p.hann, p.hann_y, W.unit(n), pad=p.pad)[0][:, y, :] for n in (0, 1)]
            for layout in (1, 2):
                basis = wp.normal_equations(*p.fdk_args(), p.weight, p.template, (y, 1), 1, p.origin, p.hann, p.hann_y, p.pad, channel_layout=layout)[2]
                for n in (0, 1):
                    differing = int((basis[n].view(np.uint32) != np.ascontiguousarray(single[n]).view(np.uint32)).sum())
                    out[f"one slice y {y} layout {layout} power {n}: differing words of {basis[n].size}"] = differing
        ramp(False)

    print(json.dumps(out, sort_keys=True))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
