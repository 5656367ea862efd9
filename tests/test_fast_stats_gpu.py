"""The diagnostic build of the FAST kernel (csrc/track_stats.hip -> libmcgpu_amd_stats.so, mode "stats"): the same text as the product kernel
with the scheduler counters woven in.  Every section-time figure of DESIGN.md and profiles/ comes from it, so it must compute what the
product computes and count what it claims to count -- under both schedulers, which share the bodies the counters sit in."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))


def test_diagnostic_build_computes_the_pinned_tallies_and_counts_the_pinned_events(engine):
    """One fresh process (the library path is fixed when the engine module is imported) runs tools/gen_fast_pin.py: compute_stats -- the
    cases catphan64_ct and tissue22 of the tally pin at their own projection, history count and seed, in mode "stats", under
    MCGPU_FAST_SCHED 0 and 1.
      - every image has the digest of tests/golden/fast_pin.json: the diagnostic build computes the product's tallies;
      - the counters that are sums over histories of events each history's own stream decides (gen_fast_pin.SCHEDULE_FREE) are the
        same under both schedulers, and equal tests/golden/fast_stats_pin.json (written by `gen_fast_pin.py --stats-pin` from the
        build BEFORE the service bodies were shared);
      - the loop and section counters are wired: iterations, scheduling points and the cycles of flight, Compton and tally + source."""
    import gen_fast_pin
    stats_lib = Path(engine.__file__).resolve().parent / "libmcgpu_amd_stats.so"
    assert stats_lib.exists(), stats_lib
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_fast_pin.py"), "--stats"], env=dict(os.environ, MCGPU_AMD_LIB=str(stats_lib)),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    pin = json.loads((ROOT / "tests" / "golden" / "fast_pin.json").read_text())
    counts = json.loads((ROOT / "tests" / "golden" / "fast_stats_pin.json").read_text())
    assert sorted(got) == sorted(gen_fast_pin.STATS_CASES) == sorted(counts)
    for name, runs in got.items():
        assert sorted(runs) == ["0", "1"]
        for sched, run in runs.items():
            s = run["stats"]
            print(name, "scheduler", sched, {k: s[k] for k in gen_fast_pin.SCHEDULE_FREE})
            assert run["sum"] == pin[name]["sum"] and run["sha256"] == pin[name]["sha256"], (name, sched)
            assert {k: s[k] for k in gen_fast_pin.SCHEDULE_FREE} == counts[name], (name, sched)
            for k in ("iterations", "scheduling_points", "cycles_flight", "cycles_compton", "cycles_new"):
                assert s[k] > 0, (name, sched, k)
        assert all(runs["0"]["stats"][k] == runs["1"]["stats"][k] for k in gen_fast_pin.SCHEDULE_FREE), name
