"""What a diagnostic tally's batch statistics cost, per batch: 100 batches of 1e6 photons on the step cloud 32 x 1 x 16 with level fluxes
and on Landsat-36 with the actinic flux (sun at mu0 = 0.5, omega = 1, black surface), two ways to the same sums on ONE handle:

  device moments   computeRadiativeTransferDiagnosticMoments (i3rc_hip_run_batches_diagnostic_moments): one call for the loop
  host loop        what a user had before that call: per batch computeRadiativeTransfer + reportResults with the diagnostic's fields,
                   x and x^2 added up in float64 on the host, the domain means included (code paths the call did not change)

The variants alternate: one warm-up round of 10 batches each, then three timed rounds; the host's clock around each loop, which ends
in a synchronous fetch either way.  The last round's sums of the two are compared (1e-9 on the fields' sums).
  python3 tools/diagnostic_moments_cost.py OUT.json [batches] [photons]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"step16": dict(switch="computeLevelFluxes", report=dict(levelFluxUp=True, levelFluxDown=True), fields=("levelFluxUp", "levelFluxDown")),
         "landsat36": dict(switch="computeActinicFlux", report=dict(actinicFlux=True), fields=("actinicFlux",))}
MU0, ROUNDS, SEED = 0.5, 3, 10


def host_loop(M, g, case, nb, n):
    s1, s2 = {}, {}
    for b in range(nb):
        g.computeRadiativeTransfer(M.new_RandomNumberSequence((SEED, 1 + b)), M.new_PhotonStream(MU0, 0.0, n))
        rep = g.reportResults(**case["report"])
        for k in case["fields"]:
            x = np.asarray(rep[k], np.float64)
            m = np.float64(np.float32(x.mean(axis=(1, 2))))
            for key, v in ((k, x), ("mean of " + k, m)):
                if key not in s1:
                    s1[key], s2[key] = np.zeros_like(v), np.zeros_like(v)
                s1[key] += v
                s2[key] += v * v
    return s1, s2


def measure(out, nb, n):
    import i3rc_monte_carlo_model_amd as M
    from tools import workloads

    record = {"what": "ms per batch of a loop of batches with a diagnostic tally's statistics: the device moments "
                      "(i3rc_hip_run_batches_diagnostic_moments) against a loop of computeRadiativeTransfer + reportResults per batch with "
                      "float64 sums on the host; the variants alternating on one handle (one warm-up round of 10 batches, three timed), "
                      "host clock around each loop; sun at mu0 = 0.5, azimuth 0, black surface, omega = 1; one MI355X. 'scatter': "
                      "(largest - smallest) / median of a row's three figures. ratio = host loop / device moments, of the medians.",
              "batches": nb, "photons_per_batch": n}
    for name, case in CASES.items():
        g, _ = workloads.make_integrator(workloads.get(name)[1])
        g.specifyParameters(**{case["switch"]: True})
        rows = {"device moments": dict(ms_per_batch=[]), "host loop": dict(ms_per_batch=[])}
        got = {}
        for rnd in range(ROUNDS + 1):                      # (round 0 warms up)
            batches = 10 if rnd == 0 else nb
            for key in rows:
                t0 = time.perf_counter()
                if key == "device moments":
                    got[key] = g.computeRadiativeTransferDiagnosticMoments((SEED, 1), batches, MU0, 0.0, n)[:2]
                else:
                    got[key] = host_loop(M, g, case, batches, n)
                ms = (time.perf_counter() - t0) * 1e3 / batches
                rows[key]["kernel"] = g.kernel_name()
                if rnd > 0:
                    rows[key]["ms_per_batch"].append(float("%.4g" % ms))
                print(name, key, "%.3f ms per batch" % ms, flush=True)
        for k in case["fields"]:
            for m in range(2):
                a, b = got["device moments"][m][k], got["host loop"][m][k]
                assert np.allclose(a, b, rtol=2e-9, atol=1e-12), (name, k, m, float(np.abs(a - b).max()))
        for r in rows.values():
            v = sorted(r["ms_per_batch"])
            r["median"] = v[len(v) // 2]
            r["scatter"] = float("%.3g" % ((v[-1] - v[0]) / r["median"]))
        rows["ratio"] = float("%.4g" % (rows["host loop"]["median"] / rows["device moments"]["median"]))
        rows["tally_block_MB"] = float("%.4g" % (g.layout().total * 8 / 1e6))
        record[name] = rows
        g.finalize_Integrator()
    json.dump(record, open(out, "w"), indent=1)


if __name__ == "__main__":
    measure(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 100, int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000)
