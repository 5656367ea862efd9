"""The cases of the scattering-sampler tests (tests/test_scatter_law.py, tests/test_scatter_gpu.py, oracle/gen_scatter_golden.py): the
smallest set that reaches every branch of the samplers.

  h2o       few shells
  blood     40 shells = the most a material may have: the widest alias table of the FAST kernels
  bone_100  high Z, strong binding: shells that cannot be ionised at low energies
  5.5 keV   just above the tables' floor: x2max = xmax^2 < xl in GRAa, and Compton products that fall below the floor
  60 keV    the middle of a CBCT spectrum
  124.5 keV just below the tables' top"""
from __future__ import annotations

import cases

MATERIALS = ("h2o", "blood", "bone_100")
ENERGIES = (5500.0, 60000.0, 124500.0)
CASES = [(m, e) for m in MATERIALS for e in ENERGIES]
SAMPLES = 1 << 20          # events per case and process, in the fixture and on the device
BINS = 64
KW = dict(n_projections=1, n_histories=1000, **cases.SMALL_DET)


def key(material: str, energy: float) -> str:
    return f"{material}_{int(energy)}"


def material_index(material: str) -> int:
    """Material number - 1: the index of the reference's tables."""
    return cases.materials.material_number(material) - 1


def build_input(out_dir):
    """A small box that holds the three materials (a context keeps tables only for materials its geometry holds)."""
    g = cases.geometry.MCBoxGeometry(shape=(12, 10, 8), image_spacing=(20.0, 20.0, 20.0), material="h2o")
    g.materials[2:5, 2:5, 2:5] = cases.materials.material_number("blood")
    g.densities[2:5, 2:5, 2:5] = 1.06
    g.materials[6:9, 5:8, 3:6] = cases.materials.material_number("bone_100")
    g.densities[6:9, 5:8, 3:6] = 1.92
    return cases.simulation.MCSimulation(g, cases.material_files(), cases.spectrum_file(), **KW).prepare_simulation(out_dir)
