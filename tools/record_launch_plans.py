#!/usr/bin/env python3
"""Records tests/golden/launch_plans.json: every row of tests/plan_sweep.py as a real one-photon launch on the device (fused rows: a
loop of one batch with fusion forced), and what the library says it decided -- i3rc_hip_last_plan and i3rc_hip_last_kernel_name, or
the refusal's text -- together with the commit it ran at.  It never asks the host-only planning entries: the file is the statement
tests/test_launch_plan_cpu.py holds them to, so it is recorded BEFORE a change of the planning code (at the parent's csrc/), and
again only by a pull request that moves a decision on purpose.

    python tools/record_launch_plans.py [OUT.json]

Stops at the first error that is not a row's expected refusal -- a HIP error above all -- and starts nothing after it."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import i3rc_monte_carlo_model_amd as M  # noqa: E402
from i3rc_monte_carlo_model_amd import binding as B  # noqa: E402
from i3rc_monte_carlo_model_amd.binding import I3RCError  # noqa: E402
from tests import plan_sweep as S  # noqa: E402

SEED = (23, 9)
FWD = 181

def _launch(g, row):
    kind, n = row["kind"], 1
    one = [np.array([v], np.float32) for v in (0.5, 0.5, 1.0, -0.7, 0.3)]   # x, y, z (relative), mu, phi of the explicit photon
    if kind == "fused":
        g.set_batch_fusion(1)
        g.computeRadiativeTransferBatches(SEED, 1, *S.SOURCE, n)
    elif kind == "replay":
        g.run_replay(M.PhotonStream(arrays=one), np.random.default_rng(1).random(4096).astype(np.float32), np.zeros(1, np.int64))
    else:
        g.set_batch_fusion(0)
        photons = M.PhotonStream(arrays=one) if row["src"] == 1 else M.new_PhotonStream(*S.SOURCE, n)
        g.computeRadiativeTransfer(M.new_RandomNumberSequence(SEED), photons)


def record(row):
    """{"name": ..., "plan": [...]} or {"refused": text}; raises on anything else"""
    d, tabs = S.domain(row["domain"])
    from tests.test_gpu_parity import make_gpu

    try:
        g = make_gpu(d, tabs)
    except I3RCError as e:
        raise SystemExit(f"{row['id']}: creating the handle failed: {e}")
    try:
        params = dict(S.PARAMS[row["params"]])
        if row["surface"]:
            del params["surfaceAlbedo"]
            params["surfaceBDRF"] = S.surface(row["surface"])
        if row["kind"] == "level":
            params["computeLevelFluxes"] = True
        if row["kind"] == "track":
            params["computeActinicFlux"] = True
        g.specifyParameters(**params)
        nd = S.directions(row["params"])
        for c, t in enumerate(tabs):
            g.set_tables(c + 1, inverse=t.inverse_table(row["inv"]), forward=t.forward_table(FWD) if nd else None)
        g.set_tuning(kernel=row["kernel"])
        g.select_grid_place(row["place"])
        g.set_lds_tallies(row["lds_tallies"])
        try:
            _launch(g, row)
        except I3RCError:
            text = g._lib.i3rc_hip_last_error(g._h).decode()
            if not row["refused"] or text.startswith("hip") or "hipError" in text:
                raise SystemExit(f"{row['id']}: {text}")
            return dict(refused=text)
        if row["refused"]:
            raise SystemExit(f"{row['id']}: expected a refusal, ran {g.kernel_name()}")
        plan = g.last_plan()
        return dict(name=g.kernel_name(), plan=[plan[k] for k in B.PLAN_NAMES])
    finally:
        g.finalize_Integrator()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "launch_plans.json")
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    commit = os.environ.get("I3RC_RECORD_COMMIT", commit)     # (a tree without its history: the caller says where it stands)
    rows = {}
    for row in S.ROWS:
        rows[row["id"]] = record(row)
        print(row["id"], rows[row["id"]].get("name") or rows[row["id"]]["refused"], flush=True)
    with open(out, "w") as f:
        f.write('{"commit": %s, "plan_names": %s, "rows": {\n' % (json.dumps(commit), json.dumps(B.PLAN_NAMES)))
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in rows.items()))
        f.write("\n}}\n")
    print(f"{len(rows)} rows -> {out}")


if __name__ == "__main__":
    main()
