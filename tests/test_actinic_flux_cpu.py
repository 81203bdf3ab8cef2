"""The actinic flux by photon track length, the parts that need no GPU: the C ABI's new symbols and the resource figures of the
kernels that tally it (photon_kernel<PhiloxTrackStream, false, true, GRID>, one per place of the extinction field)."""
import os
import sys

import i3rc_monte_carlo_model_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("i3rc_hip_set_actinic_flux", "i3rc_hip_get_actinic_flux_layout", "i3rc_hip_normalise_actinic_flux")
PLACES = ("GRID_LDS", "GRID_GLOBAL", "GRID_BRICKS", "GRID_COLUMNS", "GRID_COLBASE")


def test_actinic_flux_symbols_are_exported_and_bound():
    lib = M.binding.load()
    header = open(os.path.join(ROOT, "include", "i3rc_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in M.binding.SYMBOLS, name
        assert hasattr(lib, name), name
        assert f"int {name}(" in header, name
        assert getattr(lib, name).argtypes is not None, name


def test_actinic_flux_kernels_keep_their_state_in_registers():
    """exactly the five instantiations, and as tests/test_build_isa.py asks of the production kernels: no spilled vector register,
    no scratch"""
    sys.path.insert(0, ROOT)
    from tools.kernel_resources import resources

    rows = [r for r in resources() if "PhiloxTrackStream" in r["name"]]
    assert sorted(r["name"] for r in rows) == sorted(f"photon_kernel<PhiloxTrackStream, false, true, {p}>" for p in PLACES), [r["name"] for r in rows]
    for r in rows:
        print(r["name"], "VGPRs", r["VGPRs"], "SGPR spills", r["SGPRs Spill"], "occupancy", r["Occupancy [waves/SIMD]"])
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (r["name"], r["VGPRs Spill"], r["ScratchSize [bytes/lane]"])
