"""The one statement of the tally block's normalisation (csrc/tally_block.hpp), without a GPU: tests/normalise_main.cpp -- a host C++17
program over that header alone -- against a float64 numpy restatement of computeRadiativeTransfer :327-395, bit for bit.

The blocks are made here: positive float64 sums, whole-number counters, and excess entries that are positive, zero, and positive on
component 0 (the surface).  The sum over the columns that the redistribution divides by is formed column after column on both sides
(np.cumsum; np.sum adds pairwise).  Four cases, the smallest that reach every branch of the header: a regular grid without directions
and with the level block; the same grid with the actinic flux's block (3 x 2 x 2); an irregular grid (unequal x, y and z spacings) with
two components and two directions, contributions limited; the same block with the limit off.

The block's layout is the header's too (tally_layout): the program lays the block out from the grid sizes and the kind of the extra
block and reports the offsets and the total, which must be the ones restated here (make_block) -- in every case."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "i3rc-monte-carlo-model_amd", "csrc")
NUM_COUNTERS, CNT_PHOTONS = 16, 0    # include/i3rc_hip.h

EXTRA_NONE, EXTRA_LEVELS, EXTRA_TRACKS = 0, 1, 2    # csrc/tally_block.hpp, ExtraTally
OFFSETS = ("fluxUp", "fluxDown", "fluxAbsorbed", "volumeAbsorption", "intensityByComponent", "intensityExcess", "counters",
           "levelUp", "levelDown", "extra", "total")

REGULAR = dict(xe=[0.0, 10.0, 20.0, 30.0], ye=[0.0, 7.0, 14.0], ze=[0.0, 5.0, 10.0], ncomp=1, ndir=0, regular=1, limit=0, extra=EXTRA_LEVELS)
IRREGULAR = dict(xe=[0.0, 10.0, 25.0, 31.0], ye=[-3.0, 4.5, 9.0], ze=[0.0, 0.3, 2.0], ncomp=2, ndir=2, regular=0, limit=1, extra=EXTRA_NONE)
CASES = {"regular, level block": REGULAR, "regular, actinic block": dict(REGULAR, extra=EXTRA_TRACKS), "irregular, limit on": IRREGULAR,
         "irregular, limit off": dict(IRREGULAR, limit=0)}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("normalise") / "normalise_main"
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    subprocess.check_call([cxx, "-std=c++17", "-ffp-contract=off", "-O2", "-I", CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "normalise_main.cpp")])
    return str(exe)


def make_block(c):
    """offsets (i3rc_tally_layout, the extra block behind the counters), and a raw block"""
    nx, ny, nz, ncomp, ndir = len(c["xe"]) - 1, len(c["ye"]) - 1, len(c["ze"]) - 1, c["ncomp"], c["ndir"]
    ncol = nx * ny
    o, at = {}, 0
    for name, n in (("fluxUp", ncol), ("fluxDown", ncol), ("fluxAbsorbed", ncol), ("volumeAbsorption", ncol * nz),
                    ("intensityByComponent", (ncomp + 1) * ndir * ncol), ("intensityExcess", (ncomp + 1) * ndir), ("counters", NUM_COUNTERS)):
        o[name], at = at, at + n
    o["levelUp"] = o["levelDown"] = o["extra"] = -1
    if c["extra"] == EXTRA_LEVELS:
        o["extra"], o["levelUp"], o["levelDown"], at = at, at, at + (nz + 1) * ncol, at + 2 * (nz + 1) * ncol
    if c["extra"] == EXTRA_TRACKS:
        o["extra"], at = at, at + nz * ncol
    o["total"] = at
    rng = np.random.default_rng(20240607)
    raw = rng.uniform(0.5, 50.0, at)
    raw[o["counters"]:o["counters"] + NUM_COUNTERS] = rng.integers(1, 1000, NUM_COUNTERS)
    raw[o["counters"] + CNT_PHOTONS] = 4321.0
    if ndir:
        ex = raw[o["intensityExcess"]:o["counters"]].reshape(ncomp + 1, ndir)
        ex[:] = 0.0
        ex[0, 1], ex[2, 0] = 3.25, 0.75            # component 0 (the surface); a component; every other entry 0
        assert ex[1, 0] == 0.0
    return o, raw


def restated(c, o, raw):
    """:327-395 in float64, rounded to real(4) at the end"""
    xe, ye, ze = (np.float64(np.float32(c[k])) for k in ("xe", "ye", "ze"))
    nx, ny, nz, ncomp, ndir = len(xe) - 1, len(ye) - 1, len(ze) - 1, c["ncomp"], c["ndir"]
    ncol = nx * ny
    n_phot = raw[o["counters"] + CNT_PHOTONS]
    if c["regular"]:                                                              # :355-356
        per_col = np.full((ny, nx), n_phot / float(nx * ny))
    else:                                                                         # :358-366
        area = ((ye[1:] - ye[:-1])[:, None] * (xe[1:] - xe[:-1])[None, :]) / ((xe[-1] - xe[0]) * (ye[-1] - ye[0]))
        per_col = area * n_phot
    field = lambda name, *shape: raw[o[name]:o[name] + int(np.prod(shape))].reshape(shape).copy()
    out = [field(k, ny, nx) / per_col for k in ("fluxUp", "fluxDown", "fluxAbsorbed")]                                 # :372-374
    out.append(field("volumeAbsorption", nz, ny, nx) / (per_col[None] * (ze[1:] - ze[:-1])[:, None, None]))             # :378-381
    byc = field("intensityByComponent", ncomp + 1, ndir, ny, nx)
    excess = field("intensityExcess", ncomp + 1, ndir)
    inten = np.zeros((ndir, ny, nx))
    for j in range(ncomp + 1):                                                    # intensity: the components' sum (:574-579, :662-667)
        inten += byc[j]
    if ndir and c["limit"]:                                                       # :327-347
        for j in range(ncomp + 1):
            for d in range(ndir):
                if excess[j, d] > 0.0:
                    add = (byc[j, d] / np.cumsum(byc[j, d].ravel())[-1]) * excess[j, d]
                    inten[d] += add
                    byc[j, d] += add
    out.append(inten / per_col[None])                                             # :388
    byc[1:] /= per_col[None, None]                                                # :390-393, j = 1:numComponents
    out.append(byc)
    if c["extra"] == EXTRA_LEVELS:
        out += [field(k, nz + 1, ny, nx) / per_col[None] for k in ("levelUp", "levelDown")]
    if c["extra"] == EXTRA_TRACKS:                                                # as volumeAbsorption
        out.append(field("extra", nz, ny, nx) / (per_col[None] * (ze[1:] - ze[:-1])[:, None, None]))
    return np.concatenate([np.float32(a).ravel() for a in out])


def run(program, c, tmp_path):
    o, raw = make_block(c)
    nx, ny, nz = len(c["xe"]) - 1, len(c["ye"]) - 1, len(c["ze"]) - 1
    scalars = [nx, ny, nz, c["ncomp"], c["ndir"], c["regular"], c["limit"], c["extra"]]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array(scalars, np.int64).tobytes())
        for k in ("xe", "ye", "ze"):
            f.write(np.float32(c[k]).tobytes())
        f.write(raw.tobytes())
    subprocess.check_call([program, str(src), str(dst)])
    header = np.fromfile(dst, np.int64, len(OFFSETS))
    assert dict(zip(OFFSETS, header.tolist())) == o, (dict(zip(OFFSETS, header.tolist())), o)   # the header's layout is the one restated here
    return o, raw, np.fromfile(dst, np.float32, offset=header.nbytes)


@pytest.mark.parametrize("name", list(CASES))
def test_the_header_normalises_as_the_reference_states_it(program, name, tmp_path):
    c = CASES[name]
    o, raw, got = run(program, c, tmp_path)
    want = restated(c, o, raw)
    assert got.shape == want.shape and np.all(np.isfinite(want)) and np.all(want > 0)
    differ = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert differ.size == 0, (name, differ[:8], got[differ[:8]], want[differ[:8]])


def test_the_limit_moves_only_the_radiances_with_excess(program, tmp_path):
    """the cases reach what they are meant to reach: the limit changes the directions and components whose excess is positive, and nothing else"""
    on, off = (run(program, CASES[k], tmp_path)[2] for k in ("irregular, limit on", "irregular, limit off"))
    ncol, nz, ncomp, ndir = 6, 2, 2, 2
    first = 3 * ncol + nz * ncol
    assert np.array_equal(on[:first], off[:first])
    inten = (on[first:first + ndir * ncol] != off[first:first + ndir * ncol]).reshape(ndir, ncol)
    byc = (on[first + ndir * ncol:] != off[first + ndir * ncol:]).reshape(ncomp + 1, ndir, ncol)
    assert inten.all()                                             # (either direction has one component with excess)
    assert byc[0, 1].all() and byc[2, 0].all() and byc.sum() == 2 * ncol
