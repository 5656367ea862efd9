"""The staged detector tally (csrc/tally_stage.hpp, tally_fold.hip) against the direct atomics, bit for bit.

Integer sums commute: whichever way a detected photon reaches its tally word -- a record in the block of (workgroup, bin) that the
fold kernel sums, or the 64-bit atomic a full block falls back to -- the uint64 image is the one MCGPU_TALLY_STAGE=0 gives.  Every
case here is an ordinary launch; the reference image is computed in the same process with the staging switched off."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
KNOBS = ("MCGPU_TALLY_STAGE", "MCGPU_TALLY_STAGE_CAP", "MCGPU_TALLY_STAGE_MAX_HISTORIES")


def _set(ctx, monkeypatch, **env):
    """The staging knobs as given (others unset; staging itself forced on unless given: the default is a rule on the geometry),
    read again by the context."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict({"MCGPU_TALLY_STAGE": 1}, **env).items():
        monkeypatch.setenv(k, str(v))
    ctx.reload_env_knobs()


def _direct(ctx, monkeypatch, *args, **kw):
    _set(ctx, monkeypatch, MCGPU_TALLY_STAGE=0)
    assert ctx.geti("tally_stage_bins") == 0
    img, _, done = ctx.run_projection(*args, **kw)
    _set(ctx, monkeypatch)
    return img, done


@pytest.mark.parametrize("sched", [0, 1])
@pytest.mark.parametrize("mode", ["fast", "fast64"])
def test_staged_image_is_the_direct_image(engine, case_dir, monkeypatch, mode, sched):
    monkeypatch.setenv("MCGPU_FAST_SCHED", str(sched))
    with engine.create(case_dir("catphan64"), device=0) as ctx:
        assert ctx.geti("fast_scheduler") == sched
        n = 300_000
        ref, done = _direct(ctx, monkeypatch, 0, n, mode=mode, seed=11)
        assert done == n
        for k in range(4):
            assert int(np.count_nonzero(ref[k])) > 0, k  # all four planes: the plane bits of a record are exercised
        # default capacity: every hit is staged
        assert ctx.geti("tally_stage_bins") > 0
        f0 = ctx.geti("tally_stage_fallback_hits")
        img, _, done = ctx.run_projection(0, n, mode=mode, seed=11)
        assert done == n and np.array_equal(img, ref)
        assert ctx.geti("tally_stage_fallback_hits") == f0
        hits = ctx.geti("tally_stage_staged_hits")
        assert 0 < hits <= n and ctx.geti("tally_stage_capacity") > 0 and ctx.geti("tally_stage_bytes") > 0
        # capacity 1 (nearly every hit falls back; forced capacities are rounded up to 2) and an intermediate one
        for cap in (1, 8):
            _set(ctx, monkeypatch, MCGPU_TALLY_STAGE_CAP=cap)
            f0 = ctx.geti("tally_stage_fallback_hits")
            img, _, _ = ctx.run_projection(0, n, mode=mode, seed=11)
            fell = ctx.geti("tally_stage_fallback_hits") - f0
            print(f"mode {mode} sched {sched} cap {cap}: capacity {ctx.geti('tally_stage_capacity')}, hits {hits}, fell back {fell}, staged {ctx.geti('tally_stage_staged_hits')}")
            assert np.array_equal(img, ref), cap
            assert 0 < fell < hits and fell + ctx.geti("tally_stage_staged_hits") == hits, cap
        _set(ctx, monkeypatch)


def test_accumulation_into_an_image_that_holds_a_launch(engine, case_dir, monkeypatch):
    import torch
    with engine.create(case_dir("catphan64"), device=0) as ctx:
        a, _ = _direct(ctx, monkeypatch, 0, 100_000, mode="fast", seed=5)
        b, _ = _direct(ctx, monkeypatch, 0, 80_000, mode="fast", seed=5, first=100_000)
        assert ctx.geti("tally_stage_bins") > 0
        dev = torch.zeros(ctx.image_words, dtype=torch.int64, device="cuda:0")
        ctx.launch(0, dev.data_ptr(), 100_000, mode="fast", seed=5)
        ctx.launch(0, dev.data_ptr(), 80_000, mode="fast", seed=5, first=100_000)
        both = ctx.download_image(dev.data_ptr())
        assert np.array_equal(both, a + b) and int(a.sum()) > 0 and int(b.sum()) > 0
        ctx.launch(0, dev.data_ptr(), 100_000, mode="fast", seed=5)  # the same launch twice: twice its image
        assert np.array_equal(ctx.download_image(dev.data_ptr()), 2 * a + b)


def test_rotated_detector_pose(engine, case_dir, monkeypatch):
    with engine.create(case_dir("slab_angles"), device=0) as ctx:
        for p in range(ctx.num_projections):  # 270, 300.5 and 45.25 degrees
            ref, _ = _direct(ctx, monkeypatch, p, 60_000, mode="fast", seed=2)
            img, _, _ = ctx.run_projection(p, 60_000, mode="fast", seed=2)
            assert np.array_equal(img, ref) and int(ref.sum()) > 0, p
        assert ctx.geti("tally_stage_fallback_hits") == 0


@pytest.mark.parametrize("sched", [0, 1])
def test_launches_smaller_than_a_workgroup(engine, case_dir, monkeypatch, sched):
    """Waves that find no work at all still reach the kernel's final barrier: 1, 63 and 1025 histories leave most waves of the grid
    (1, 63) or of the second workgroup (1025) without a history.  A count of 0 launches no kernel: it covers the host path only."""
    monkeypatch.setenv("MCGPU_FAST_SCHED", str(sched))
    with engine.create(case_dir("water"), device=0) as ctx:
        for n in (0, 1, 63, 1025):
            ref, done = _direct(ctx, monkeypatch, 0, n, mode="fast", seed=3, first=17)
            img, _, d = ctx.run_projection(0, n, mode="fast", seed=3, first=17)
            assert d == done == n and np.array_equal(img, ref), n
        assert int(ref.sum()) > 0


def test_sub_launches_give_the_unsplit_image(engine, case_dir, monkeypatch):
    with engine.create(case_dir("catphan64"), device=0) as ctx:
        n = 60_000
        ref, _ = _direct(ctx, monkeypatch, 0, n, mode="fast", seed=8, first=2 ** 32 - 1000)
        whole, _, _ = ctx.run_projection(0, n, mode="fast", seed=8, first=2 ** 32 - 1000)
        _set(ctx, monkeypatch, MCGPU_TALLY_STAGE_MAX_HISTORIES=7001)
        split, _, done = ctx.run_projection(0, n, mode="fast", seed=8, first=2 ** 32 - 1000)
        _set(ctx, monkeypatch)
        assert done == n and np.array_equal(whole, ref) and np.array_equal(split, ref)


@pytest.mark.parametrize("stage", [None, 1])
def test_a_refused_stats_launch_leaves_the_context_usable(engine, case_dir, monkeypatch, stage):
    """The product library carries no diagnostic kernel: a "stats" launch is refused -- after the launch has prepared its staging
    buffers -- and the context goes on giving the image it gave before.  Default knobs and staging forced on."""
    if "stats" in Path(engine.LIB_PATH).name:
        pytest.skip("MCGPU_AMD_LIB points at the diagnostic library, which runs the stats mode")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if stage is not None:
        monkeypatch.setenv("MCGPU_TALLY_STAGE", str(stage))
    with engine.create(case_dir("catphan64"), device=0) as ctx:
        ref, _, done = ctx.run_projection(0, 20_000, mode="fast", seed=3)
        assert done == 20_000 and int(ref.sum()) > 0
        with pytest.raises(engine.EngineError) as e:
            ctx.run_projection(0, 20_000, mode="stats", seed=3)
        assert e.value.code == -2 and "libmcgpu_amd_stats.so" in e.value.message
        again, _, _ = ctx.run_projection(0, 20_000, mode="fast", seed=3)
        assert np.array_equal(again, ref)


def test_dose_tallies_share_the_final_barrier(engine, case_dir, monkeypatch):
    with engine.create(case_dir("catphan64_dose"), device=0) as ctx:
        assert ctx.dose_info()[0] == 3
        ctx.dose_clear()
        ref, _ = _direct(ctx, monkeypatch, 0, 60_000, mode="fast", seed=4)
        vox_ref, mat_ref = ctx.dose_read()
        ctx.dose_clear()
        assert ctx.geti("tally_stage_bins") > 0
        img, _, _ = ctx.run_projection(0, 60_000, mode="fast", seed=4)
        vox, mat = ctx.dose_read()
        assert np.array_equal(img, ref)
        assert np.array_equal(vox, vox_ref) and np.array_equal(mat, mat_ref) and int(mat_ref.sum()) > 0 and int(vox_ref.sum()) > 0


def test_bench_tally_is_the_direct_one(tmp_path):
    """A plain bench.py run: the tally of its last timed step (--dump-outputs) with MCGPU_TALLY_STAGE=1 (what the default rule picks for
    this geometry) against MCGPU_TALLY_STAGE=0, the direct atomics of the same build -- textually the parent's tally path; the parent
    commit itself cannot be run from inside this tree."""
    out = {}
    for stage in ("1", "0"):
        env = dict(os.environ, MCGPU_TALLY_STAGE=stage)
        env.pop("MCGPU_TALLY_STAGE_CAP", None)
        d = tmp_path / f"stage{stage}"
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["value"] > 0
        out[stage] = {f.name: np.load(f) for f in sorted(d.glob("*.npy"))}
        assert out[stage], "bench.py --dump-outputs wrote nothing"
    assert out["1"].keys() == out["0"].keys()
    for name in out["1"]:
        assert np.array_equal(out["1"][name], out["0"][name]), name
    assert any(float(v.sum()) > 0 for v in out["1"].values())
