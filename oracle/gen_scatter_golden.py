#!/usr/bin/env python3
"""Histograms of the reference's scattering samplers -> tests/golden/scatter_law.npz (test infrastructure).

For every case of tests/scatter_cases.py: 2^20 calls of oracle_gcoa and 2^20 of oracle_graa (LIBM math: the mode that
tests/test_oracle_golden.py pins call by call to the reference build), binned.  The file holds counts and sums only:
  <case>_co_edges / _co_cos    cos(theta) of Compton events: bin edges, counts
  <case>_co_tedges / _co_tau   E'/E: bin edges, counts
  <case>_co_tsum / _co_tsq     sum of E'/E and of its square per cos(theta) bin (mean and standard error of the mean)
  <case>_co_low                events whose product lies below the tables' lowest energy
  <case>_ra_edges / _ra_cos    cos(theta) of Rayleigh events
Bin edges are the 64-quantiles of an independent pilot run (2^18 events, other seed), so that every bin expects about 2^14 events;
edges that coincide (an atom of the distribution, such as E'/E = 1) are merged.  The first and last edge are -inf / +inf."""
import ctypes as C
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT))
import cases, oracle_lib as ol, parity, scatter_cases as sc, scatter_ref  # noqa: E402

PILOT = 1 << 18


def stream(batch, seed):
    s = (C.c_int * 2)()
    ol.oracle().oracle_init_prng(batch, 150, seed, s)
    return s


def gcoa(T, mat, energy, n, s):
    e_out, cos = np.zeros(n, dtype=np.float32), np.zeros(n)
    ol.oracle().oracle_gcoa_many(C.byref(T.ct), float(energy), mat, s, ol.MATH_LIBM, n, e_out.ctypes.data, cos.ctypes.data)
    return e_out.astype(np.float64) / np.float64(np.float32(energy)), cos, e_out


def graa(T, mat, energy, index, n, s):
    cos = np.zeros(n)
    ol.oracle().oracle_graa_many(C.byref(T.ct), float(energy), mat, index, s, n, cos.ctypes.data)
    return cos


def quantile_edges(v, bins):
    e = np.unique(np.quantile(v, np.linspace(0, 1, bins + 1)[1:-1]))
    return np.concatenate([[-np.inf], e, [np.inf]])


def main():
    out = {}
    with tempfile.TemporaryDirectory() as wd:
        with cases.pkg.engine.create(sc.build_input(Path(wd)), device=-1) as ctx:
            T = parity.tables_from_context(ctx)
            tab = scatter_ref.tables(ctx)
            for k, (material, energy) in enumerate(sc.CASES):
                mat, name = sc.material_index(material), sc.key(material, energy)
                index = scatter_ref.energy_index(tab, energy)
                tau_p, cos_p, _ = gcoa(T, mat, energy, PILOT, stream(2 * k, 4242))
                edges, tedges = quantile_edges(cos_p, sc.BINS), quantile_edges(tau_p, sc.BINS)
                tau, cos, e_out = gcoa(T, mat, energy, sc.SAMPLES, stream(2 * k + 1, 977))
                b = np.searchsorted(edges, cos, side="right") - 1
                out[name + "_co_edges"], out[name + "_co_tedges"] = edges, tedges
                out[name + "_co_cos"] = np.bincount(b, minlength=edges.size - 1).astype(np.int64)
                out[name + "_co_tau"] = np.histogram(tau, tedges)[0].astype(np.int64)
                out[name + "_co_tsum"] = np.bincount(b, weights=tau, minlength=edges.size - 1)
                out[name + "_co_tsq"] = np.bincount(b, weights=tau * tau, minlength=edges.size - 1)
                out[name + "_co_low"] = np.int64(np.count_nonzero(e_out < tab["e0"]))
                redges = quantile_edges(graa(T, mat, energy, index, PILOT, stream(2 * k, 5151)), sc.BINS)
                out[name + "_ra_edges"] = redges
                out[name + "_ra_cos"] = np.histogram(graa(T, mat, energy, index, sc.SAMPLES, stream(2 * k + 1, 1313)), redges)[0].astype(np.int64)
                assert min(out[name + "_co_cos"].min(), out[name + "_co_tau"].min(), out[name + "_ra_cos"].min()) >= 100, name
                print(name, "bins", edges.size - 1, tedges.size - 1, redges.size - 1, "below the floor", int(out[name + "_co_low"]), flush=True)
    out["samples"] = np.int64(sc.SAMPLES)
    np.savez_compressed(ROOT / "tests" / "golden" / "scatter_law.npz", **out)


if __name__ == "__main__":
    main()
