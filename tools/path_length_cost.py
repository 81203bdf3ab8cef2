"""What the path-length moments (i3rc_hip_set_path_lengths) cost: photons per second of plain flux launches on the step cloud
32 x 1 x 16 (the benchmark's domain: sun at the zenith, omega = 1, black surface), the variants alternating on ONE handle -- one
warm-up round, three timed, device events around each launch -- with the run's own work counters.
  python3 tools/path_length_cost.py OUT.json          this build: every diagnostic off (the general kernel), level fluxes on, path lengths on
  I3RC_LIB=other.so python3 tools/path_length_cost.py OUT.json    another build of the library (the parent commit's, in a process of its
                                                       own): the general kernel and level fluxes on
  python3 tools/path_length_cost.py --merge THIS.json PARENT.json OUT.json    the two records in one file, with the ratios"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOAD, PHOTONS, ROUNDS = "step16", 200_000_000, 3


def measure(out):
    import i3rc_monte_carlo_model_amd as M

    other = os.environ.get("I3RC_LIB")
    if other:
        M.build.LIB = os.path.abspath(other); M.build.needs_build = lambda: False
    from tools import workloads

    w = workloads.get(WORKLOAD)[1]
    g, _ = workloads.make_integrator(w)
    g.set_tuning(kernel="general")
    has_feature = not other and hasattr(g._lib, "i3rc_hip_set_path_lengths")
    variants = {"off, general kernel": {}, "level fluxes on": dict(computeLevelFluxes=True)}
    if has_feature:
        variants["path lengths on"] = dict(computePathLengths=True)
    rows = {k: dict(photons_per_s=[]) for k in variants}
    for rnd in range(ROUNDS + 1):                      # (round 0 warms up)
        for key, switch in variants.items():
            g.specifyParameters(**switch)
            res = g.computeRadiativeTransfer(M.new_RandomNumberSequence((10, 1 + rnd)), M.new_PhotonStream(w["mu0"], 0.0, PHOTONS))
            ms = g.kernel_ms()
            r, c = rows[key], res["counters"]
            r["kernel"] = g.kernel_name()
            r["steps_per_photon"] = round(c["cellSteps"] / c["photons"], 3)
            r["scatterings_per_photon"] = round(c["scatterings"] / c["photons"], 3)
            if rnd > 0:
                r["photons_per_s"].append(float("%.4g" % (PHOTONS / ms * 1e3)))
            if "pathLengthUp" in res:                  # the two domain mean paths of the run, in the domain's length unit
                lay = g.layout()
                offs = g.path_length_layout()
                ncol = g.nx * g.ny
                raw = res["raw"]
                r["mean_path_up"] = float("%.6g" % (raw[offs[0]:offs[0] + ncol].sum() / raw[lay.fluxUp:lay.fluxUp + ncol].sum()))
                r["mean_path_down"] = float("%.6g" % (raw[offs[2]:offs[2] + ncol].sum() / raw[lay.fluxDown:lay.fluxDown + ncol].sum()))
            print(key, r["kernel"], "%.2f ms" % ms, flush=True)
            g.specifyParameters(**{k: False for k in switch})
    for r in rows.values():
        v = sorted(r["photons_per_s"])
        r["median"] = v[len(v) // 2]
        r["scatter"] = float("%.3g" % ((v[-1] - v[0]) / r["median"]))
    g.finalize_Integrator()
    json.dump({"library": "parent" if other else "this", "photons": PHOTONS, WORKLOAD: rows}, open(out, "w"), indent=1)


def merge(this, parent, out):
    t, p = json.load(open(this)), json.load(open(parent))
    rec = {"what": "photons per second of plain flux launches on the step cloud 32 x 1 x 16 (sun at the zenith, omega = 1, black surface) with "
                   "every diagnostic tally off (the general flux kernel), with level fluxes on and with path lengths on, same handle, rounds "
                   "alternating the variants (one warm-up round, three timed), device events around each launch; one MI355X. 'parent': the "
                   "parent commit's library in a process of its own, same script, without the path lengths it does not have. 'scatter': "
                   "(largest - smallest) / median of a row's three figures.",
           "photons_per_launch": t["photons"], "this": t[WORKLOAD], "parent": p[WORKLOAD], "ratios": {}}
    paths = t[WORKLOAD]["path lengths on"]["median"]
    rec["ratios"]["path lengths on / parent's level fluxes on"] = float("%.4g" % (paths / p[WORKLOAD]["level fluxes on"]["median"]))
    rec["ratios"]["path lengths on / level fluxes on"] = float("%.4g" % (paths / t[WORKLOAD]["level fluxes on"]["median"]))
    rec["ratios"]["path lengths on / off, general kernel"] = float("%.4g" % (paths / t[WORKLOAD]["off, general kernel"]["median"]))
    for key in ("off, general kernel", "level fluxes on"):
        rec["ratios"][f"{key}: this / parent"] = float("%.4g" % (t[WORKLOAD][key]["median"] / p[WORKLOAD][key]["median"]))
    json.dump(rec, open(out, "w"), indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(*sys.argv[2:5])
    else:
        measure(sys.argv[1])
