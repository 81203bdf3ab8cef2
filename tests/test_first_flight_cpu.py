"""The first flight of a zenith sun's photons from a column table (csrc/first_flight.hpp): where a photon that goes straight down its
start column has its first event, found by a search in the column's cumulative optical path instead of voxel step after voxel step.
No GPU: tests/first_flight_main.cpp -- a host C++17 program over the header alone, which the kernels include too, built with
-ffp-contract=off as the library is -- holds first_flight_landing to a sequential restatement of the vertical trace (the step, the test
`acc + step * ext > t`, the arrival's division), everything compared with ==: steps, layer, and the height bit for bit.  Its columns:
1 ... 64 layers of equal and of unequal depths, clear layers above, inside and below the cloud, all-clear columns, extinctions from
1e-30 to 1e4; its depths: every A[k] itself, the floats on both sides of it, points between two sums, depths beyond A[nz], random ones.

first_flight_eligible is held to its sentence, restated here, over a grid of all its inputs:

  a plain launch of a STORE kernel, a Directional source, solarDx == 0 and solarDy == 0 with either sign of zero, the start layer in
  1 .. nz, nx <= 2047, ny <= 2047, nz <= 1022, and the table exists

-- and solarDz == -1, which the sentence implies (upload_source makes solarDz = -|mu| of a unit vector) and the function holds the
launch to, since the landing's faces are those of a photon that goes down."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = M.build.CSRC


def build_program(d, extra):
    exe = d / "first_flight_main"
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    subprocess.check_call([cxx, "-std=c++17", "-ffp-contract=off", "-O2", *extra, "-I", CSRC, "-o", str(exe),
                           os.path.join(ROOT, "tests", "first_flight_main.cpp")])
    return str(exe)


def counts_of(exe):
    p = subprocess.run([exe, "landing"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode in (0, 1), p.stderr
    words = p.stdout.split()
    return dict(zip(words[0::2], (int(v) for v in words[1::2]))), p.stderr


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_program(tmp_path_factory.mktemp("first_flight"), [])


@pytest.fixture(scope="module")
def landing(program):
    return counts_of(program)


def test_the_landing_is_the_vertical_trace(landing):
    n, err = landing
    assert n["cases"] > 100000
    assert n["mismatches"] == 0, err


def test_the_cases_cover_what_the_issue_names(landing):
    n, _ = landing
    assert n["columns"] == 1500
    for what in ("bottom", "landed", "firstStep", "lastLayer", "onTable", "beyond", "clearAbove", "clearInside", "clearBelow", "allClear", "unequal",
                 "tinyExt", "hugeExt", "lands", "notLands"):
        assert n[what] > 0, what
    assert n["onTable"] > 1500 * 2           # (t == A[k], for every k of every column; the float on each side of it with it)
    assert n["unequal"] == 750               # every other column has layers of unequal depths


def test_an_elevated_domain_whose_start_rounds_to_the_top_is_ineligible(program):
    words = subprocess.run([program, "elevated"], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    got = dict(zip(words[0::2], words[1::2]))
    assert float.fromhex(got["zStart"]) == float.fromhex(got["zMax"]) == 4097.0
    assert int(got["layer"]) == int(got["nz"]) + 1
    assert got["eligible"] == "0"


def test_eligibility_is_its_sentence(program):
    out = subprocess.run([program, "eligible"], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    rows = [r.split() for r in out if r]
    assert len(rows) == 2 * 2 * 5 * 5 * 3 * 3 * 3 * 3 * 4 * 2
    yes = 0
    for store, src, dx, dy, dz, start, nx, ny, nz, table, got in rows:
        dx, dy, dz = (np.array(int(v, 16), np.uint32).view(np.float32) for v in (dx, dy, dz))
        start, nx, ny, nz = int(start), int(nx), int(ny), int(nz)
        want = (store == "1" and src == "0" and bool(dx == 0) and bool(dy == 0) and bool(dz == -1) and 1 <= start <= nz
                and nx <= 2047 and ny <= 2047 and nz <= 1022 and table == "1")
        assert (got == "1") == want, (store, src, dx, dy, dz, start, nx, ny, nz, table, got)
        yes += want
    assert yes == 2 * 2 * 2 * 2 * (2 + 2)   # (either sign of zero on both axes; nx and ny within the packing; nz = 1: start 1, listed twice, nz = 1022: 1 and nz)


def test_the_slot_packing_round_trips_at_its_limits(program):
    """ix | iy << 11 | code << 22 taken apart again: the indices up to 2047, the codes 0 (through the bottom), 1 ... 1022 (a layer) and 1023
    (not landed); one 32-bit word, no field reaching into its neighbour; the launch's bit is none of EventFlag's"""
    rows = [r.split() for r in subprocess.run([program, "pack"], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n") if r]
    limits = [int(v) for v in rows.pop()[1:]]
    assert limits == [2047, 1022, 0, 1023, 16]
    assert len(rows) == 4 * 4 * 5
    seen = set()
    for ix, iy, code, word, gx, gy, gc in rows:
        assert (ix, iy, code) == (gx, gy, gc), (ix, iy, code, word)
        assert int(word, 16) == int(ix) | int(iy) << 11 | int(code) << 22 < 2 ** 32
        seen.add(word)
    assert len(seen) == len(rows)                       # (distinct inputs, distinct words)
    assert {"2047"} <= {r[0] for r in rows} & {r[1] for r in rows} and {"0", "1022", "1023"} <= {r[2] for r in rows}
    flags = [int(m) for m in re.findall(r"= (\d+)u,", open(os.path.join(CSRC, "event_flags.hpp")).read())]
    assert flags and 16 not in flags and all(f < 16 for f in flags)


def test_the_program_under_the_sanitizers_says_the_same(landing, tmp_path):
    exe = build_program(tmp_path, ["-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"])
    n, err = counts_of(exe)
    assert n == landing[0], err
    subprocess.run([exe, "elevated"], stdout=subprocess.DEVNULL, check=True)
    subprocess.run([exe, "eligible"], stdout=subprocess.DEVNULL, check=True)
    subprocess.run([exe, "pack"], stdout=subprocess.DEVNULL, check=True)
