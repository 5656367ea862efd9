"""Respiratory phase of a breathing curve, for the phase-sorted 4-D reconstruction (`reconstruction.reconstruct_4d`).

What it must reproduce is the reference's phase (its peak finder and `calculate_phase`), so the rules below are the reference's
behaviour, written down and implemented here from that description; tests/test_rooster4d.py pins peaks and phase against recorded
reference outputs (tests/golden/reference_phase_cases.npz).  Nothing here needs scipy.

Peaks -- AMPD (automatic multiscale-based peak detection, Scholkmann et al. 2012, in the form that also finds peaks near the
ends of the curve):
  1. remove the least-squares straight line from the curve (a linear detrend);
  2. for every scale k = 1..K, K = n // 2 (or `scale` if smaller), sample i is a k-maximum when it is strictly larger than the
     samples at i - k and i + k that exist (a missing neighbour beyond an end does not count against it);
  3. weight the number of k-maxima by n // 2 - k + 1 (fewer samples have both neighbours at large k) and take the first scale
     index lam (0-based) with the largest weighted count;
  4. a peak is a sample that is a k-maximum for every k = 1..lam.

Phase (`calculate_phase`, phase_range (a, b)):
  - peaks as above; then the edge rule is `if ... elif`: a peak on the first sample is dropped, and only when there is none, a
    peak on the last sample (a curve with peaks on both ends keeps the last one);
  - between consecutive peaks p < q the phase runs linearly from a at p to b at q - 1 (n = q - p points);
  - the part before the first peak and the part from the last peak on take the phase of the median cycle, M = its length samples
    from a to b, repeated as often as needed: the first part ends with the end of that sequence, the last part starts with its start;
  - the median cycle: the curve split at its peaks (here the edge rule drops end peaks on BOTH ends), the pieces whose length lies
    within one population standard deviation of the median piece length, each resampled linearly to int(median length) samples,
    and their sample-wise median;
  - the phase is float32 (computed in float64, then stored), and it is returned split at the peaks (np.hstack joins it).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np


def detrend_linear(x) -> np.ndarray:
    """x minus the least-squares line through (i, x[i])."""
    y = np.asarray(x, dtype=np.float64)
    t = np.arange(y.size, dtype=np.float64)
    tc = t - t.mean()
    slope = float(tc @ (y - y.mean())) / float(tc @ tc) if y.size > 1 else 0.0
    return y - (y.mean() + slope * tc)


def _local_maxima(y: np.ndarray, k: int) -> np.ndarray:
    """Samples strictly above their neighbours at distance k (where those exist)."""
    m = np.ones(y.size, dtype=bool)
    m[:-k] &= y[:-k] > y[k:]
    m[k:] &= y[k:] > y[:-k]
    return m


def find_peaks(x, scale: int = None, debug: bool = False):
    """Peak indices (ascending) of a quasi-periodic noisy curve by AMPD (module docstring).  debug=True returns
    (peaks, maxima [K][n] bool, weighted counts [K], lam)."""
    y = detrend_linear(x)
    n = y.size
    K = n // 2 if not scale else min(scale, n // 2)
    maxima = np.array([_local_maxima(y, k) for k in range(1, K + 1)]).reshape(K, n)
    weighted = maxima.sum(axis=1) * (n // 2 - np.arange(K))
    lam = int(np.argmax(weighted))
    if lam == 0:
        raise ValueError("find_peaks: no scale with persistent maxima (curve too short or flat)")
    peaks = np.flatnonzero(np.logical_and.reduce(maxima[:lam], axis=0))
    return (peaks, maxima, weighted, lam) if debug else peaks


@dataclass
class RespiratoryStatistics:
    mean_cycle_period: float
    median_cycle_period: float
    std_cycle_period: float
    n_complete_cycles: float
    mean_cycle_span: float
    std_cycle_span: float
    total_length_secs: float


def split_into_cycles(curve, peaks=None) -> List[np.ndarray]:
    """The curve cut at its peaks; peaks on the first or the last sample do not cut."""
    curve = np.asarray(curve)
    peaks = np.asarray(find_peaks(curve) if peaks is None else peaks)
    cuts = peaks[(peaks != 0) & (peaks != curve.size - 1)]
    return np.split(curve, cuts)


def calculate_respiratory_statistics(amplitudes, sampling_rate: float = 1.0) -> RespiratoryStatistics:
    """Length (seconds at `sampling_rate`) and span statistics of the pieces of split_into_cycles."""
    pieces = split_into_cycles(amplitudes)
    lengths = np.array([p.size for p in pieces], dtype=np.float64) / sampling_rate
    spans = np.array([np.max(p) - np.min(p) for p in pieces])
    return RespiratoryStatistics(float(lengths.mean()), float(np.median(lengths)), float(lengths.std()), len(pieces),
                                 float(spans.mean()), float(spans.std()), float(lengths.sum()))


def calculate_median_cycle(curve) -> np.ndarray:
    """Sample-wise median of the typical pieces, each resampled to the median piece length (module docstring)."""
    st = calculate_respiratory_statistics(curve)
    lo, hi = st.median_cycle_period - st.std_cycle_period, st.median_cycle_period + st.std_cycle_period
    m = int(st.median_cycle_period)
    stretched = [np.interp(np.linspace(0, p.size - 1, m), np.arange(p.size), p) for p in split_into_cycles(curve) if lo <= p.size <= hi]
    return np.median(stretched, axis=0)


def calculate_phase(breathing_curve, phase_range: Tuple[float, float] = (0, 2 * math.pi)) -> List[np.ndarray]:
    """Phase of every sample, float32, split at the peaks (module docstring)."""
    curve = np.asarray(breathing_curve)
    n = curve.size
    peaks = [int(p) for p in find_peaks(curve)]
    if peaks[0] == 0:
        del peaks[0]
    elif peaks[-1] == n - 1:
        del peaks[-1]
    a, b = phase_range
    phase = np.full(n, np.nan, dtype=np.float32)
    for p, q in zip(peaks, peaks[1:]):
        phase[p:q] = np.linspace(a, b, q - p)
    ramp = np.linspace(a, b, len(calculate_median_cycle(curve)))
    head, tail = peaks[0], n - peaks[-1]
    ramp = np.tile(ramp, math.ceil(max(head, tail) / ramp.size))
    phase[:head] = ramp[ramp.size - head:]
    phase[n - tail:] = ramp[:tail]
    return np.split(phase, peaks)
