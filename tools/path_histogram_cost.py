"""What the path-length histogram (i3rc_hip_set_path_histogram) costs: photons per second of plain flux launches on the step cloud
32 x 1 x 16 (the benchmark's domain: sun at the zenith, omega = 1, black surface), the variants alternating on ONE handle -- one
warm-up round, three timed, device events around each launch -- with the run's own work counters.
  python3 tools/path_histogram_cost.py OUT.json          this build: every diagnostic off (the general kernel), path lengths on, the
                                                          histogram with 64 and with 1024 bins (sums in LDS) and with its sums forced
                                                          to global memory (64 bins)
  I3RC_LIB=other.so python3 tools/path_histogram_cost.py OUT.json    another build of the library (the parent commit's, in a process
                                                          of its own): the general kernel and path lengths on
  python3 tools/path_histogram_cost.py --merge THIS.json PARENT.json OUT.json    the two records in one file, with the ratios"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOAD, PHOTONS, ROUNDS = "step16", 200_000_000, 3
OFF, PATHS = "off, general kernel", "path lengths on"
BINS64, BINS1024, GLOBAL64 = "histogram, 64 bins, sums in LDS", "histogram, 1024 bins, sums in LDS", "histogram, 64 bins, global atomics"


def edges(nbins):
    """from a hundredth of the cloud's 250 m in geometric progression to 1e6 m: the overflow bin stays empty"""
    return np.concatenate([[0.0], np.geomspace(2.5, 1e6, nbins)]).astype(np.float32)


def measure(out):
    import i3rc_monte_carlo_model_amd as M

    other = os.environ.get("I3RC_LIB")
    if other:
        M.build.LIB = os.path.abspath(other); M.build.needs_build = lambda: False
    from tools import workloads

    w = workloads.get(WORKLOAD)[1]
    g, _ = workloads.make_integrator(w)
    g.set_tuning(kernel="general")
    has_feature = not other and hasattr(g._lib, "i3rc_hip_set_path_histogram")
    # (switch on, LDS sums, switch off)
    variants = {OFF: ({}, True, {}), PATHS: (dict(computePathLengths=True), True, dict(computePathLengths=False))}
    if has_feature:
        variants[BINS64] = (dict(pathHistogramEdges=edges(64)), True, dict(pathHistogramEdges=None))
        variants[BINS1024] = (dict(pathHistogramEdges=edges(1024)), True, dict(pathHistogramEdges=None))
        variants[GLOBAL64] = (dict(pathHistogramEdges=edges(64)), False, dict(pathHistogramEdges=None))
    rows = {k: dict(photons_per_s=[]) for k in variants}
    for rnd in range(ROUNDS + 1):                      # (round 0 warms up)
        for key, (on, lds, off) in variants.items():
            g.specifyParameters(**on)
            g.set_lds_tallies(lds)
            res = g.computeRadiativeTransfer(M.new_RandomNumberSequence((10, 1 + rnd)), M.new_PhotonStream(w["mu0"], 0.0, PHOTONS))
            ms = g.kernel_ms()
            r, c = rows[key], res["counters"]
            r["kernel"] = g.kernel_name()
            r["steps_per_photon"] = round(c["cellSteps"] / c["photons"], 3)
            r["scatterings_per_photon"] = round(c["scatterings"] / c["photons"], 3)
            if rnd > 0:
                r["photons_per_s"].append(float("%.4g" % (PHOTONS / ms * 1e3)))
            if "pathHistogramUp" in res:               # which launch it was, and the two domain mean paths the bins give
                r["sums_in_lds"] = g.last_plan()[M.binding.PLAN_BIN_NAME]
                r["overflow"] = float(res["pathHistogramUp"][-1] + res["pathHistogramDown"][-1])
                up, pup, down, pdown = (res[k].astype(np.float64) for k in M.host.PATH_HISTOGRAM_NAMES)
                r["mean_path_up"], r["mean_path_down"] = float("%.6g" % (pup.sum() / up.sum())), float("%.6g" % (pdown.sum() / down.sum()))
            print(key, r["kernel"], "%.2f ms" % ms, flush=True)
            g.set_lds_tallies(True)
            g.specifyParameters(**off)
    for r in rows.values():
        v = sorted(r["photons_per_s"])
        r["median"] = v[len(v) // 2]
        r["scatter"] = float("%.3g" % ((v[-1] - v[0]) / r["median"]))
    g.finalize_Integrator()
    json.dump({"library": "parent" if other else "this", "photons": PHOTONS, WORKLOAD: rows}, open(out, "w"), indent=1)


def merge(this, parent, out):
    t, p = json.load(open(this)), json.load(open(parent))
    rec = {"what": "photons per second of plain flux launches on the step cloud 32 x 1 x 16 (sun at the zenith, omega = 1, black surface) with "
                   "every diagnostic tally off (the general flux kernel), with path lengths on, and with the path histogram on: 64 and "
                   "1024 bins with the workgroups' sums in LDS, 64 bins with the sums forced to global atomics (i3rc_hip_set_lds_tallies(h, 0), "
                   "which sends the flux tallies there too); same handle, rounds alternating the variants (one warm-up round, three timed), "
                   "device events around each launch; one MI355X. 'parent': the parent commit's library in a process of its own, same "
                   "script, without the histogram it does not have. 'scatter': (largest - smallest) / median of a row's three figures.",
           "photons_per_launch": t["photons"], "this": t[WORKLOAD], "parent": p[WORKLOAD], "ratios": {}}
    T, P = t[WORKLOAD], p[WORKLOAD]
    yard = P[PATHS]
    for key in (BINS64, BINS1024, GLOBAL64):
        rec["ratios"][f"{key} / parent's path lengths on"] = float("%.4g" % (T[key]["median"] / yard["median"]))
        rec["ratios"][f"{key} / off, general kernel"] = float("%.4g" % (T[key]["median"] / T[OFF]["median"]))
    rec["ratios"]["64 bins: sums in LDS / global atomics"] = float("%.4g" % (T[BINS64]["median"] / T[GLOBAL64]["median"]))
    for key in (OFF, PATHS):
        rec["ratios"][f"{key}: this / parent"] = float("%.4g" % (T[key]["median"] / P[key]["median"]))
    # the yardstick: the parent's launch with path lengths on, less three times the larger scatter of the two rows
    for key in (BINS64, BINS1024):
        floor = yard["median"] * (1 - 3 * max(yard["scatter"], T[key]["scatter"]))
        rec["ratios"][f"{key}: reaches the parent's path-lengths launch less three scatters"] = bool(T[key]["median"] >= floor)
    json.dump(rec, open(out, "w"), indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(*sys.argv[2:5])
    else:
        measure(sys.argv[1])
