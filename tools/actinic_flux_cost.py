"""What the actinic flux (i3rc_hip_set_actinic_flux) costs: photons per second of plain flux launches on the step cloud 32 x 1 x 16
and on Landsat-36 (sun at mu0 = 0.5, omega = 1, black surface), the variants alternating on ONE handle -- one warm-up round, three
timed, device events around each launch -- with the run's own work counters (voxel steps and scatterings per photon = float64
atomics per photon of the feature).
  python3 tools/actinic_flux_cost.py OUT.json          this build: feature off (the kernel a launch chooses; the general kernel), feature
                                                       on with sums in LDS (where the field lies in LDS) and with global atomics
  ACTINIC_OFF_ONLY=1 python3 tools/actinic_flux_cost.py OUT.json   this build, the feature-off variants alone: the sequence the parent's runs
  I3RC_LIB=other.so python3 tools/actinic_flux_cost.py OUT.json    another build of the library (the parent commit's, in a process of its
                                                       own): the feature-off variants only
  python3 tools/actinic_flux_cost.py --merge THIS.json PARENT.json OUT.json    the two records in one file, with the scatter of the
                                                       feature-off rows"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"step16": 50_000_000, "landsat36": 20_000_000}
MU0, ROUNDS = 0.5, 3


def measure(out):
    import i3rc_monte_carlo_model_amd as M

    other = os.environ.get("I3RC_LIB")
    if other:
        M.build.LIB = os.path.abspath(other); M.build.needs_build = lambda: False
    from tools import workloads

    record = {"library": "parent" if other else "this"}
    for name, n in SIZES.items():
        g, _ = workloads.make_integrator(workloads.get(name)[1])
        # (ACTINIC_OFF_ONLY=1: this build through the parent's sequence -- the feature-off variants alone)
        has_feature = not other and not os.environ.get("ACTINIC_OFF_ONLY") and hasattr(g._lib, "i3rc_hip_set_actinic_flux")

        def variant(kernel, on, lds):
            g.set_tuning(kernel=kernel)
            g.set_lds_tallies(lds)
            if has_feature:
                g.specifyParameters(computeActinicFlux=on)

        variants = {"off, kernel chosen": ("auto", False, True), "off, general kernel": ("general", False, True)}
        if has_feature:
            variants["on, sums in LDS"] = ("auto", True, True)
            variants["on, global atomics"] = ("auto", True, False)
        rows = {k: dict(photons_per_s=[]) for k in variants}
        for rnd in range(ROUNDS + 1):                      # (round 0 warms up)
            for key, (kernel, on, lds) in variants.items():
                variant(kernel, on, lds)
                res = g.computeRadiativeTransfer(M.new_RandomNumberSequence((10, 1 + rnd)), M.new_PhotonStream(MU0, 0.0, n))
                ms = g.kernel_ms()
                rows[key]["kernel"] = g.kernel_name()
                rows[key]["lds_track_sums"] = g.last_plan().get("ldsTrackSums", 0)
                c = res["counters"]
                rows[key]["steps_per_photon"] = round(c["cellSteps"] / c["photons"], 3)
                rows[key]["scatterings_per_photon"] = round(c["scatterings"] / c["photons"], 3)
                if rnd > 0:
                    rows[key]["photons_per_s"].append(float("%.4g" % (n / ms * 1e3)))
                print(name, key, rows[key]["kernel"], "%.2f ms" % ms, flush=True)
        for key, r in rows.items():
            v = sorted(r["photons_per_s"])
            r["median"] = v[len(v) // 2]
            r["scatter"] = float("%.3g" % ((v[-1] - v[0]) / r["median"]))
            if r["kernel"].startswith("photon_kernel<PhiloxTrackStream"):
                r["atomics_per_photon"] = round(r["steps_per_photon"] + r["scatterings_per_photon"], 3)
                r["atomics_per_s"] = float("%.4g" % (r["median"] * r["atomics_per_photon"]))
        if has_feature and rows["on, sums in LDS"]["lds_track_sums"] == 0:
            del rows["on, sums in LDS"]                      # (the field is not in LDS: the variant was the global one once more)
        rows["photons"] = n
        record[name] = rows
        g.finalize_Integrator()
    json.dump(record, open(out, "w"), indent=1)


def merge(this, parent, out):
    t, p = json.load(open(this)), json.load(open(parent))
    rec = {"what": "photons per second of plain flux launches with the actinic flux on and off, same handle, rounds alternating the variants "
                   "(one warm-up round, three timed), device events around each launch; sun at mu0 = 0.5, azimuth 0, black surface, omega = 1; "
                   "one MI355X. 'parent': the parent commit's library in a process of its own, same script, the feature-off variants. "
                   "'scatter': (largest - smallest) / median of a row's three figures. atomics_per_photon = voxel steps + scatterings "
                   "per photon from the run's own counters.",
           "sizes": {k: f"{v} photons per launch" for k, v in SIZES.items()}, "this": t, "parent": p, "ratios": {}}
    for name in SIZES:
        gen = t[name]["off, general kernel"]["median"]
        for key in ("on, sums in LDS", "on, global atomics"):
            if key in t[name]:
                rec["ratios"][f"{name} {key} / off general"] = float("%.4g" % (t[name][key]["median"] / gen))
        for key in ("off, kernel chosen", "off, general kernel"):
            rec["ratios"][f"{name} {key}: this / parent"] = float("%.4g" % (t[name][key]["median"] / p[name][key]["median"]))
    json.dump(rec, open(out, "w"), indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(*sys.argv[2:5])
    else:
        measure(sys.argv[1])
