"""The biased-base form of a cell's address (csrc/cell_address.hpp), which the photon step of the specialised flux kernels of plain
launches reads its extinction through: the three `- 1` of the 1-based indices and the field's base folded into one launch-uniform bias,
  bias = base - 4 (nx ny + nx + 1),   address = (((iz nx ny + ix) + iy nx) << 2) + bias.
No GPU: tests/cell_address_main.cpp -- a host C++17 program over the header alone, which the kernels include too -- against
  4 cell_index + base,   cell_index = (iz - 1) nx ny + (iy - 1) nx + (ix - 1)      (tracer.hpp),
modulo 2^32, worked out here in Python integers, for

  every cell of 1 x 1 x 1, 1 x 1 x 16, 32 x 1 x 16 (the step cloud), 3 x 5 x 7 and 64 x 64 x 2;
  the eight corner cells of 4095 x 4097 x 64: nx ny = 2^24 - 1, the largest the 24-bit multiplies take, and 2^30 - 64 cells, just under
  the 2^30 the library accepts -- the sum in front of the shift passes 2^30 there and wraps with it;
  base 0 and 4 -- both below 4 (nx ny + nx + 1) of every grid, 12 for the single cell: the bias is negative as an int --, a base as a
  field has it in LDS behind the edges, and the low word of a global address just under 2^32.

cell_word (the sum in front of the shift: what the global-memory form indexes a moved base with, and the event phase takes its cell index
from) must exceed cell_index by nx ny + nx + 1 exactly, without wrapping; column_address is the same folding for the [ny][nx] records of
8 bytes that the column-record kernels read: ((iy - 1) nx + (ix - 1)) * 8 + base."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import i3rc_monte_carlo_model_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = M.build.CSRC
M32 = (1 << 32) - 1

EVERY_CELL = [(1, 1, 1), (1, 1, 16), (32, 1, 16), (3, 5, 7), (64, 64, 2)]
LARGE = (4095, 4097, 64)


def bases(nx, ny, nz):
    return [0, 4, 4 * (nx + ny + nz + 3), 0xFFFFFFF0]


def records():
    """(base, nx, ny, ix, iy, iz) of every case, and where each grid's records with each base lie in the list"""
    out, where = [], {}
    for nx, ny, nz in EVERY_CELL:
        for base in bases(nx, ny, nz):
            where[base, nx, ny, nz] = len(out)
            out += [(base, nx, ny, ix, iy, iz) for iz in range(1, nz + 1) for iy in range(1, ny + 1) for ix in range(1, nx + 1)]
    nx, ny, nz = LARGE
    for base in bases(nx, ny, nz):
        out += [(base, nx, ny, ix, iy, iz) for iz, iy, ix in itertools.product((1, nz), (1, ny), (1, nx))]
    return out, where


@pytest.fixture(scope="module")
def computed(tmp_path_factory):
    d = tmp_path_factory.mktemp("cell_address")
    exe = d / "cell_address_main"
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    subprocess.check_call([cxx, "-std=c++17", "-ffp-contract=off", "-O2", "-I", CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "cell_address_main.cpp")])
    recs, where = records()
    src, dst = d / "in.bin", d / "out.bin"
    np.array(recs, np.uint32).tofile(src)
    subprocess.check_call([str(exe), str(src), str(dst)])
    out = np.fromfile(dst, np.uint32)
    assert out.size == 5 * len(recs)
    return recs, out.reshape(-1, 5), where


def test_the_large_grid_is_at_the_limits():
    nx, ny, nz = LARGE
    assert nx * ny == (1 << 24) - 1 and (1 << 30) - 2 * nx * ny < nx * ny * nz < 1 << 30
    assert nx * ny * nz + nx * ny + nx + 1 > 1 << 30        # (the sum in front of the shift passes 2^30: its top bits leave with the shift)
    assert all(n < 1 << 24 for n in LARGE)


def test_address_equals_four_cell_index_plus_base(computed):
    recs, out, where = computed
    negative = 0
    for (base, nx, ny, ix, iy, iz), (bias, addr, word, _, _) in zip(recs, out):
        cell = (iz - 1) * nx * ny + (iy - 1) * nx + (ix - 1)
        what = (base, nx, ny, ix, iy, iz)
        assert int(bias) == (base - 4 * (nx * ny + nx + 1)) & M32, what
        assert int(addr) == (4 * cell + base) & M32, what
        assert int(word) == cell + nx * ny + nx + 1, what       # (no wrap: below 2^31)
        negative += base < 4 * (nx * ny + nx + 1) and int(bias) >= 1 << 31
    assert negative > 0     # (the bias that is negative as an int occurs: base 0 and 4 of every grid)
    for nx, ny, nz in EVERY_CELL:   # every cell of the small grids, each base: as many records as cells, no address twice
        for base in bases(nx, ny, nz):
            first = where[base, nx, ny, nz]
            got = sorted(int(a) for a in out[first:first + nx * ny * nz, 1])
            if base + 4 * nx * ny * nz <= M32:
                assert got == list(range(base, base + 4 * nx * ny * nz, 4)), (base, nx, ny, nz)
            else:
                assert len(set(got)) == nx * ny * nz, (base, nx, ny, nz)


def test_column_address_equals_eight_column_index_plus_base(computed):
    recs, out, _ = computed
    for (base, nx, ny, ix, iy, iz), (_, _, _, bias, addr) in zip(recs, out):
        assert int(bias) == (base - 8 * (nx + 1)) & M32, (base, nx)
        assert int(addr) == (8 * ((iy - 1) * nx + (ix - 1)) + base) & M32, (base, nx, ny, ix, iy)
