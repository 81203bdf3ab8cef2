"""ctypes binding of the C ABI declared in include/i3rc_hip.h.

There is no CPU fallback: if the HIP library is missing or no GPU is present, calls fail loudly."""
import ctypes as C
import os

import numpy as np

from . import build as _build

fp = C.POINTER(C.c_float)
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int32)
lp = C.POINTER(C.c_int64)
up = C.POINTER(C.c_uint32)

MAX_COMPONENTS = 255
MAX_DIRECTIONS = 255
NUM_COUNTERS = 16
COUNTER_NAMES = ["photons", "dropped", "cellSteps", "scatterings", "surfaceHits", "exitsTop", "roulette",
                 "shadowSteps", "tracerCalls", "rngDraws", "raysSkipped"]

# every symbol include/i3rc_hip.h declares (checked by tests/test_host_cpu.py::test_cabi_library_exports_every_declared_symbol)
SYMBOLS = [
    "i3rc_hip_create", "i3rc_hip_destroy", "i3rc_hip_last_error", "i3rc_hip_set_inverse_table",
    "i3rc_hip_set_forward_tables", "i3rc_hip_set_params", "i3rc_hip_set_surface", "i3rc_hip_set_directions",
    "i3rc_hip_get_tally_layout", "i3rc_hip_bind_tally_buffer", "i3rc_hip_set_stream", "i3rc_hip_use_own_stream", "i3rc_hip_zero_tallies",
    "i3rc_hip_launch_batch", "i3rc_hip_run_batches", "i3rc_hip_run_batches_moments", "i3rc_hip_get_moments_layout", "i3rc_hip_compute_batch", "i3rc_hip_expect_batches", "i3rc_hip_run_replay", "i3rc_hip_trace_rays", "i3rc_hip_synchronize",
    "i3rc_hip_fetch_tallies", "i3rc_hip_normalise", "i3rc_hip_last_kernel_ms", "i3rc_hip_kernel_ms_history", "i3rc_hip_set_tuning", "i3rc_hip_force_general_kernel", "i3rc_hip_select_kernel", "i3rc_hip_set_light_threshold", "i3rc_hip_set_first_flight_table", "i3rc_hip_last_first_flight", "i3rc_hip_set_launch_limit",
    "i3rc_hip_set_batch_fusion", "i3rc_hip_select_grid_place", "i3rc_hip_has_column_records", "i3rc_hip_column_records", "i3rc_hip_column_records_base", "i3rc_hip_lds_plan", "i3rc_hip_lds_plan_words", "i3rc_hip_set_lds_tallies", "i3rc_hip_last_kernel_name", "i3rc_hip_last_plan", "i3rc_hip_timed_launch_count", "i3rc_hip_philox_blocks", "i3rc_hip_arith_check", "i3rc_hip_find_index", "i3rc_hip_surface_reflectance", "i3rc_hip_device_count", "i3rc_hip_version",
    "i3rc_hip_set_level_fluxes", "i3rc_hip_get_level_flux_layout", "i3rc_hip_normalise_level_fluxes",
    "i3rc_hip_set_actinic_flux", "i3rc_hip_get_actinic_flux_layout", "i3rc_hip_normalise_actinic_flux",
    "i3rc_hip_set_path_lengths", "i3rc_hip_get_path_length_layout", "i3rc_hip_normalise_path_lengths",
    "i3rc_hip_set_path_histogram", "i3rc_hip_get_path_histogram_layout", "i3rc_hip_normalise_path_histogram",
    "i3rc_hip_set_radiance_path_lengths", "i3rc_hip_get_radiance_path_length_layout", "i3rc_hip_normalise_radiance_path_lengths",
    "i3rc_hip_problem_facts", "i3rc_hip_plan_launch",
    "i3rc_hip_run_batches_diagnostic_moments", "i3rc_hip_get_diagnostic_moments_layout", "i3rc_hip_diagnostic_moments_layout_words",
    "i3rc_hip_set_path_spectrum", "i3rc_hip_get_path_moments_layout", "i3rc_hip_path_moments_layout_words", "i3rc_hip_run_batches_path_moments",
]


class Params(C.Structure):
    _fields_ = [
        ("surfaceAlbedo", C.c_float), ("useSurfaceBDRF", C.c_int32), ("useRayTracing", C.c_int32),
        ("useRussianRoulette", C.c_int32), ("useHybridPhaseFunsForIntenCalcs", C.c_int32),
        ("numOrdersOrigPhaseFunIntenCalcs", C.c_int32), ("useRussianRouletteForIntensity", C.c_int32),
        ("zetaMin", C.c_float), ("limitIntensityContributions", C.c_int32), ("maxIntensityContribution", C.c_float),
    ]


class Source(C.Structure):
    _fields_ = [("kind", C.c_int32), ("solarMu", C.c_float), ("solarAzimuth", C.c_float),
                ("x", fp), ("y", fp), ("z", fp), ("mu", fp), ("phi", fp)]


class TallyLayout(C.Structure):
    _fields_ = [("fluxUp", C.c_int64), ("fluxDown", C.c_int64), ("fluxAbsorbed", C.c_int64),
                ("volumeAbsorption", C.c_int64), ("intensityByComponent", C.c_int64), ("intensityExcess", C.c_int64),
                ("counters", C.c_int64), ("total", C.c_int64)]


class MomentsLayout(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("fluxUp", "fluxDown", "fluxAbsorbed", "volumeAbsorption", "intensity", "absorbedProfile",
                                         "meanFluxUp", "meanFluxDown", "meanFluxAbsorbed", "meanIntensity", "total")]


# i3rc_diagnostic_moments_layout; without its first word, the words of i3rc_hip_diagnostic_moments_layout_words in order
DIAGNOSTIC_MOMENTS_NAMES = ["levelFluxUp", "levelFluxDown", "meanLevelFluxUp", "meanLevelFluxDown", "actinicFlux", "meanActinicFlux", "total"]
EXTRA_KINDS = {"none": 0, "levels": 1, "tracks": 2, "paths": 3, "bins": 4, "radiance_paths": 5}   # (the radiance path lengths have no batch moments yet; csrc/tally_block.hpp, ExtraTally; path lengths and the path histogram have their batch moments in a layout of their own, path_moments_layout below)
MAX_PATH_BINS = 1024   # (csrc/tally_block.hpp, kMaxPathBins)


class DiagnosticMomentsLayout(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ["kind"] + DIAGNOSTIC_MOMENTS_NAMES]


def diagnostic_moments_layout(kind, nx, ny, nz, nout=len(DIAGNOSTIC_MOMENTS_NAMES)):
    """i3rc_hip_diagnostic_moments_layout_words: a dict of DIAGNOSTIC_MOMENTS_NAMES for a kind (EXTRA_KINDS, or its number) and a grid.
    No device needed."""
    out = (C.c_int64 * max(int(nout), 1))()
    if load().i3rc_hip_diagnostic_moments_layout_words(int(EXTRA_KINDS.get(kind, kind)), int(nx), int(ny), int(nz), out, int(nout)) != 0:
        raise I3RCError("i3rc_hip_diagnostic_moments_layout_words: bad arguments")
    return dict(zip(DIAGNOSTIC_MOMENTS_NAMES, (int(v) for v in out)))


# i3rc_path_moments_layout; without its first three words, the words of i3rc_hip_path_moments_layout_words in order
PATH_MOMENTS_NAMES = ["pathLengthUp", "pathLengthSquaredUp", "pathLengthDown", "pathLengthSquaredDown",
                      "meanPathLengthUp", "meanPathLengthSquaredUp", "meanPathLengthDown", "meanPathLengthSquaredDown",
                      "domainPathUp", "domainPathSquaredUp", "domainPathDown", "domainPathSquaredDown",
                      "histogramUp", "histogramPathUp", "histogramDown", "histogramPathDown",
                      "spectrumUpLower", "spectrumUpUpper", "spectrumDownLower", "spectrumDownUpper", "total"]
MAX_PATH_SPECTRUM = 256   # (csrc/tally_block.hpp, kMaxPathSpectrum)


class PathMomentsLayout(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ["kind", "nBins", "nK"] + PATH_MOMENTS_NAMES]


def path_moments_layout(kind, nx, ny, nBins=0, nK=0, nout=len(PATH_MOMENTS_NAMES)):
    """i3rc_hip_path_moments_layout_words: a dict of PATH_MOMENTS_NAMES for a kind ("paths" / "bins", or its number), a grid, the
    histogram's bins and the spectrum's coefficients.  No device needed."""
    out = (C.c_int64 * max(int(nout), 1))()
    if load().i3rc_hip_path_moments_layout_words(int(EXTRA_KINDS.get(kind, kind)), int(nx), int(ny), int(nBins), int(nK), out, int(nout)) != 0:
        raise I3RCError("i3rc_hip_path_moments_layout_words: bad arguments")
    return dict(zip(PATH_MOMENTS_NAMES, (int(v) for v in out)))


# the words of i3rc_hip_last_plan, in order
PLAN_NAMES = ["ldsGrid", "ldsTallies", "ldsVolume", "ldsIntensity", "tableInLds", "ldsBytes", "absorbing", "cellRecordBytes",
              "fusedBatches", "place", "startStoreBytes", "chunk", "ldsTrackSums"]
# ... and the fourteenth, which the call hands out where it is asked for: the path histogram's sums and edges in LDS (1), or its block
# added to in global memory (0)
PLAN_BIN_NAME = "ldsPathBins"


# the words of i3rc_hip_problem_facts, in order ...
FACT_NAMES = ["nx", "ny", "nz", "ncomp", "xyRegular", "zRegular", "empty", "absorbing", "uniformSsa", "uniformPf", "cellRecordBytes",
              "columnRecords", "columnBase", "bsx", "bsy", "bsz", "nbx", "nby", "nbz", "clearShift", "clearNx", "clearWords", "maxPfIndex"]
# ... and of i3rc_hip_plan_launch: what the setters and the handle's knobs add to them, the switches of the process (with their
# defaults), the kinds of stream, and what follows the words of PLAN_NAMES in its answer
SETUP_NAMES = ["nDir", "inverseTables", "forwardTables", "inverseSteps", "inverseEntries", "useSurfaceBDRF", "useRayTracing", "surfaceNx",
               "surfaceNy", "surfaceSet", "extra", "kernelVariant", "gridPlace", "ldsTalliesOn"]
ENV_DEFAULTS = {"I3RC_COLUMNS": 1, "I3RC_LDS_TALLIES": 1, "I3RC_TABLE_LDS": 1, "I3RC_TABLE_LDS_PLACES": 11, "I3RC_FUSED_TABLE_LDS_PLACES": 11,
                "I3RC_DIRECT": 1, "I3RC_CELL_RECORDS": 1}
STREAM_KINDS = {"plain": 0, "fused": 1, "replay": 2, "level": 3, "track": 4, "path": 5, "bins": 6, "radiance_path": 7}
PLAN_EXTRA_NAMES = ["ldsEstimate", "rayQueueCap", "threads"]


def _env_words(env):
    """the switches of the process as i3rc_hip_problem_facts / i3rc_hip_plan_launch take them: None (the process's own), or a dict of
    ENV_DEFAULTS' names over their defaults"""
    if env is None:
        return None
    unknown = set(env) - set(ENV_DEFAULTS)
    if unknown:
        raise KeyError(f"not a switch a launch reads: {sorted(unknown)}")
    return (C.c_int32 * len(ENV_DEFAULTS))(*[int(env.get(k, v)) for k, v in ENV_DEFAULTS.items()])


def problem_facts(nx, ny, nz, ncomp, xe, ye, ze, total, cum, ssa, pfi, env=None):
    """i3rc_hip_problem_facts on the arrays of i3rc_hip_create (float32 / int32, contiguous): a dict of FACT_NAMES.  No device needed."""
    out = (C.c_int32 * len(FACT_NAMES))()
    rc = load().i3rc_hip_problem_facts(nx, ny, nz, ncomp, pf(xe), pf(ye), pf(ze), pf(total), pf(cum), pf(ssa), pfi.ctypes.data_as(ip),
                                       _env_words(env), out, len(FACT_NAMES))
    if rc != 0:
        raise I3RCError("i3rc_hip_problem_facts: " + (load().i3rc_hip_last_error(None).decode() if rc == 1 else "bad arguments"))
    return dict(zip(FACT_NAMES, (int(v) for v in out)))


def plan_launch(facts, setup, stream="plain", source=0, fused_batches=0, env=None, path_bins=0):
    """i3rc_hip_plan_launch: (kernel name, dict of PLAN_NAMES + PLAN_EXTRA_NAMES), or (refusal text, None).  facts: a dict of FACT_NAMES;
    setup: a dict of SETUP_NAMES.  stream "bins" (the path histogram): path_bins its bins, and PLAN_BIN_NAME one more word of the dict.
    No device needed."""
    bins = stream == "bins"
    n = len(PLAN_NAMES) + len(PLAN_EXTRA_NAMES) + int(bins)
    out, text = (C.c_int32 * n)(), C.create_string_buffer(512)
    rc = load().i3rc_hip_plan_launch((C.c_int32 * len(FACT_NAMES))(*[int(facts[k]) for k in FACT_NAMES]),
                                     (C.c_int32 * len(SETUP_NAMES))(*[int(setup[k]) for k in SETUP_NAMES]), _env_words(env),
                                     (C.c_int32 * 4)(STREAM_KINDS[stream], int(source), int(fused_batches), int(path_bins)), out, n, text,
                                     len(text))
    if rc == 2:
        raise I3RCError("i3rc_hip_plan_launch: bad arguments")
    names = PLAN_NAMES + PLAN_EXTRA_NAMES + ([PLAN_BIN_NAME] if bins else [])
    return text.value.decode(), (dict(zip(names, (int(v) for v in out))) if rc == 0 else None)


class I3RCError(RuntimeError):
    pass


_lib = None


def library_path():
    return _build.LIB


def load():
    """Load csrc/libi3rc_hip.so; raise (never fall back) if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise I3RCError(f"{path} not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                        "the integrator has no CPU fallback")
    L = C.CDLL(path)
    H = C.c_void_p
    L.i3rc_hip_create.argtypes = [C.POINTER(H), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, fp, fp, fp, fp, ip]
    L.i3rc_hip_destroy.argtypes = [H]
    L.i3rc_hip_last_error.argtypes = [H]
    L.i3rc_hip_last_error.restype = C.c_char_p
    L.i3rc_hip_set_inverse_table.argtypes = [H, C.c_int, C.c_int, C.c_int, fp]
    L.i3rc_hip_set_forward_tables.argtypes = [H, C.c_int, C.c_int, C.c_int, fp, fp]
    L.i3rc_hip_set_params.argtypes = [H, C.POINTER(Params)]
    L.i3rc_hip_set_surface.argtypes = [H, C.c_int, C.c_int, fp, fp, fp]
    L.i3rc_hip_set_directions.argtypes = [H, C.c_int, fp]
    L.i3rc_hip_get_tally_layout.argtypes = [H, C.POINTER(TallyLayout)]
    L.i3rc_hip_bind_tally_buffer.argtypes = [H, C.c_void_p, C.c_size_t]
    L.i3rc_hip_set_stream.argtypes = [H, C.c_void_p]
    L.i3rc_hip_use_own_stream.argtypes = [H]
    L.i3rc_hip_zero_tallies.argtypes = [H]
    L.i3rc_hip_launch_batch.argtypes = [H, C.c_uint32, C.c_uint32, C.c_int64, C.c_int64, C.POINTER(Source)]
    if hasattr(L, "i3rc_hip_run_batches"):   # (absent from older builds loaded for A/B timing)
        L.i3rc_hip_run_batches.argtypes = [H, C.c_uint32, C.c_uint32, C.c_int, C.c_int64, C.POINTER(Source), C.c_int, dp]
    if hasattr(L, "i3rc_hip_run_batches_moments"):
        L.i3rc_hip_run_batches_moments.argtypes = [H, C.c_uint32, C.c_uint32, C.c_int, C.c_int64, C.POINTER(Source), dp, dp, dp]
        L.i3rc_hip_get_moments_layout.argtypes = [H, C.POINTER(MomentsLayout)]
    if hasattr(L, "i3rc_hip_expect_batches"):
        L.i3rc_hip_expect_batches.argtypes = [H, C.c_uint32, C.c_uint32, C.c_int, C.c_int64, C.POINTER(Source), C.POINTER(C.c_int)]
    if hasattr(L, "i3rc_hip_compute_batch"):
        L.i3rc_hip_compute_batch.argtypes = [H, C.c_uint32, C.c_uint32, C.c_int64, C.POINTER(Source), C.c_int, dp]
    L.i3rc_hip_run_replay.argtypes = [H, C.c_int64, C.POINTER(Source), fp, C.c_int64, lp, ip, ip, fp, ip, ip]
    L.i3rc_hip_trace_rays.argtypes = [H, C.c_int64, fp, fp, ip, fp, fp, ip]
    L.i3rc_hip_synchronize.argtypes = [H]
    L.i3rc_hip_fetch_tallies.argtypes = [H, dp]
    L.i3rc_hip_normalise.argtypes = [H, dp, fp, fp, fp, fp, fp, fp]
    L.i3rc_hip_last_kernel_ms.argtypes = [H, fp]
    L.i3rc_hip_kernel_ms_history.argtypes = [H, C.c_int, fp]
    if hasattr(L, "i3rc_hip_last_kernel_name"):   # (absent from older builds of the library loaded for A/B timing: tools/lib_compare.py)
        L.i3rc_hip_last_kernel_name.argtypes = [H]
        L.i3rc_hip_timed_launch_count.argtypes = [H]
        L.i3rc_hip_timed_launch_count.restype = C.c_int64
        L.i3rc_hip_last_kernel_name.restype = C.c_char_p
    if hasattr(L, "i3rc_hip_last_plan"):
        L.i3rc_hip_last_plan.argtypes = [H, ip, C.c_int]
    L.i3rc_hip_set_tuning.argtypes = [H, C.c_int, C.c_int]
    L.i3rc_hip_force_general_kernel.argtypes = [H, C.c_int]
    L.i3rc_hip_select_kernel.argtypes = [H, C.c_int]
    L.i3rc_hip_set_light_threshold.argtypes = [H, C.c_int]
    if hasattr(L, "i3rc_hip_set_first_flight_table"):   # (an older build of the library, loaded for an A/B comparison, has neither)
        L.i3rc_hip_set_first_flight_table.argtypes = [H, C.c_int]
        L.i3rc_hip_last_first_flight.argtypes = [H]
    L.i3rc_hip_set_launch_limit.argtypes = [H, C.c_int64]
    if hasattr(L, "i3rc_hip_set_batch_fusion"):
        L.i3rc_hip_set_batch_fusion.argtypes = [H, C.c_int]
    if hasattr(L, "i3rc_hip_select_grid_place"):
        L.i3rc_hip_select_grid_place.argtypes = [H, C.c_int]
        L.i3rc_hip_has_column_records.argtypes = [H]
        L.i3rc_hip_column_records.argtypes = [C.c_int, C.c_int, C.c_int, fp, up]
    if hasattr(L, "i3rc_hip_column_records_base"):
        L.i3rc_hip_column_records_base.argtypes = [C.c_int, C.c_int, C.c_int, fp, up, fp]
    if hasattr(L, "i3rc_hip_lds_plan"):
        L.i3rc_hip_lds_plan.argtypes = [ip, ip]
        L.i3rc_hip_set_lds_tallies.argtypes = [H, C.c_int]
    if hasattr(L, "i3rc_hip_lds_plan_words"):   # (absent from older builds loaded for A/B timing)
        L.i3rc_hip_lds_plan_words.argtypes = [ip, C.c_int, ip, C.c_int]
    L.i3rc_hip_philox_blocks.argtypes = [H, C.c_uint32, C.c_uint32, C.c_int64, C.c_int64, C.c_int, up, fp]
    L.i3rc_hip_arith_check.argtypes = [H, C.c_int64, fp, fp, lp, lp]
    if hasattr(L, "i3rc_hip_find_index"):
        L.i3rc_hip_find_index.argtypes = [H, C.c_int, fp, C.c_int64, fp, ip, ip]
        L.i3rc_hip_surface_reflectance.argtypes = [H, C.c_int64, fp, fp, fp]
    if hasattr(L, "i3rc_hip_set_level_fluxes"):   # (absent from older builds loaded for A/B timing)
        L.i3rc_hip_set_level_fluxes.argtypes = [H, C.c_int]
        L.i3rc_hip_get_level_flux_layout.argtypes = [H, lp, lp, lp]
        L.i3rc_hip_normalise_level_fluxes.argtypes = [H, dp, fp, fp]
    if hasattr(L, "i3rc_hip_set_actinic_flux"):   # (likewise)
        L.i3rc_hip_set_actinic_flux.argtypes = [H, C.c_int]
        L.i3rc_hip_get_actinic_flux_layout.argtypes = [H, lp, lp]
        L.i3rc_hip_normalise_actinic_flux.argtypes = [H, dp, fp]
    if hasattr(L, "i3rc_hip_set_path_lengths"):   # (likewise)
        L.i3rc_hip_set_path_lengths.argtypes = [H, C.c_int]
        L.i3rc_hip_get_path_length_layout.argtypes = [H, lp, lp, lp, lp, lp]
        L.i3rc_hip_normalise_path_lengths.argtypes = [H, dp, fp, fp, fp, fp]
    if hasattr(L, "i3rc_hip_set_path_histogram"):   # (likewise)
        L.i3rc_hip_set_path_histogram.argtypes = [H, C.c_int, fp]
        L.i3rc_hip_get_path_histogram_layout.argtypes = [H, lp, lp, lp, lp, lp, lp]
        L.i3rc_hip_normalise_path_histogram.argtypes = [H, dp, fp, fp, fp, fp]
    if hasattr(L, "i3rc_hip_set_radiance_path_lengths"):   # (likewise)
        L.i3rc_hip_set_radiance_path_lengths.argtypes = [H, C.c_int]
        L.i3rc_hip_get_radiance_path_length_layout.argtypes = [H, lp, lp, lp]
        L.i3rc_hip_normalise_radiance_path_lengths.argtypes = [H, dp, fp, fp]
    if hasattr(L, "i3rc_hip_plan_launch"):   # (likewise)
        L.i3rc_hip_problem_facts.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, fp, fp, fp, fp, ip, ip, ip, C.c_int]
        L.i3rc_hip_plan_launch.argtypes = [ip, ip, ip, ip, ip, C.c_int, C.c_char_p, C.c_int]
    if hasattr(L, "i3rc_hip_run_batches_diagnostic_moments"):   # (likewise)
        L.i3rc_hip_run_batches_diagnostic_moments.argtypes = [H, C.c_uint32, C.c_uint32, C.c_int, C.c_int64, C.POINTER(Source), dp, dp, dp, dp, dp]
        L.i3rc_hip_get_diagnostic_moments_layout.argtypes = [H, C.POINTER(DiagnosticMomentsLayout)]
        L.i3rc_hip_diagnostic_moments_layout_words.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, lp, C.c_int]
    if hasattr(L, "i3rc_hip_run_batches_path_moments"):   # (likewise)
        L.i3rc_hip_set_path_spectrum.argtypes = [H, C.c_int, fp]
        L.i3rc_hip_get_path_moments_layout.argtypes = [H, C.POINTER(PathMomentsLayout)]
        L.i3rc_hip_path_moments_layout_words.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, lp, C.c_int]
        L.i3rc_hip_run_batches_path_moments.argtypes = [H, C.c_uint32, C.c_uint32, C.c_int, C.c_int64, C.POINTER(Source), dp, dp, dp, dp, dp]
    L.i3rc_hip_device_count.restype = C.c_int
    L.i3rc_hip_version.restype = C.c_char_p
    _lib = L
    return L


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def pf(a):
    return a.ctypes.data_as(fp)
