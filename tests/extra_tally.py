"""What the two suites of the optional diagnostic tally share (tests/test_gpu_level_fluxes.py, tests/test_gpu_actinic_flux.py): their
domains, the recipes of the general flux kernel's five places, and how they run a batch.  A plain module beside tests/kernel_matrix.py."""
import numpy as np

import i3rc_monte_carlo_model_amd as M
from tests import kernel_matrix as K

f32 = np.float32
N = 30_001          # a multiple of neither the 256-photon chunk nor a workgroup

PLACES = list(zip(K.PLACES, ("two", "three", "step_records", "columns2", "colbase2")))   # the general flux kernel's recipes
IRREGULAR_Z = np.array([0.0, 12.0, 40.0, 47.0, 90.0, 131.0, 160.0, 233.0, 250.0], np.float32)   # 8 irregular layers


def run(g, n=N, *, seed, sun=K.SOURCE):
    return g.computeRadiativeTransfer(M.new_RandomNumberSequence(seed), M.new_PhotonStream(sun[0], sun[1], n))


def old(g, res):
    """the tallies the handle had before the feature: everything in front of the counters"""
    return res["raw"][:g.layout().counters]


def step_cloud_3d(ssa):
    """8 x 4 x 6 cells, step-cloud-like: thin and thick columns in x, a modulation in y, a clear layer on top"""
    nx, ny, nz = 8, 4, 6
    col = np.where(np.arange(nx) < nx // 2, 2.0, 18.0)[None, :] * np.array([1.0, 0.5, 1.5, 0.25])[:, None] / 250.0
    ext = np.ascontiguousarray(np.broadcast_to(col[None], (nz, ny, nx)), np.float32).copy()
    ext[nz - 1] = 0.0
    pf = (ext > 0).astype(np.int32)
    return dict(xe=f32(62.5) * np.arange(nx + 1, dtype=np.float32), ye=f32(125.0) * np.arange(ny + 1, dtype=np.float32),
                ze=np.array([0.0, 30.0, 80.0, 120.0, 170.0, 210.0, 250.0], np.float32), ext=ext,
                ssa=np.where(ext > 0, f32(ssa), f32(0)).astype(np.float32), pf=pf)
