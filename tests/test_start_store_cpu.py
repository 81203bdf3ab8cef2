"""The start stores in the carve-up of a workgroup's LDS (csrc/tracer.hpp lds_plan, asked through i3rc_hip_lds_plan_words: host code,
no device): where they lie for workgroups of 256 and of 1024 threads, that nothing overlaps them, and that a carve-up without them is
the one it always was."""
import numpy as np

STORE_WORDS_PER_WAVE = 4 * 64   # StartSlot: four words a slot, 64 slots


def _plan(lib, B, nx, ny, nz, place, tallies, volume, table, store):
    waves = 16 if table else 4
    clear_nx, clear_shift = (nx + 3) // 4, 2
    q = np.array([nx, ny, nz, 1, 0, tallies, 0, 0, clear_nx, clear_shift, 0, 0, place, 0, waves, table, volume, store], np.int32)
    out = np.full(13, -7, np.int32)
    assert lib.i3rc_hip_lds_plan_words(q.ctypes.data_as(B.ip), len(q), out.ctypes.data_as(B.ip), len(out)) == 0
    return [int(v) for v in out], waves


def test_start_store_in_the_lds_carve_up():
    from i3rc_monte_carlo_model_amd import binding as B

    lib = B.load()
    rng = np.random.default_rng(11)
    shapes = [(32, 1, 16), (4, 1, 3), (5, 3, 2), (1, 1, 1), (7, 3, 9), (33, 2, 13)] + [tuple(int(v) for v in rng.integers(1, 40, 3)) for _ in range(40)]
    for nx, ny, nz in shapes:
        for place in (0, 1, 3):                      # (the bricked kernels have no store)
            for tallies, volume in ((0, 0), (1, 0), (1, 1)):
                for table in (0, 10001):             # 256 threads | 1024 threads with the inverse table's cosines
                    out, waves = _plan(lib, B, nx, ny, nz, place, tallies, volume, table, 1)
                    xE, yE, zE, tal, dirs, dirtab, queue, tint, ext, costab, end, tvol, store = out
                    ncol = nx * ny
                    size = waves * STORE_WORDS_PER_WAVE
                    assert size * 4 == (16 if table else 4) * 1024
                    assert store % 4 == 0, out                                     # 128-bit reads of a slot
                    # the regions in the order of the carve-up: none overlaps the next, the store among them
                    regions = [(xE, nx + 1), (yE, ny + 1), (zE, nz + 1), (tal, 4 * ncol if tallies else 0), (tvol, 2 * ncol * nz if volume else 0),
                               (dirs, 0), (dirtab, 0), (queue, 0), (tint, 0), (ext, ncol * nz if place == 0 else 0), (store, size), (costab, table)]
                    at = 0
                    for off, words in regions:
                        assert off >= at, (out, off, at)
                        at = off + words
                    assert at == end, out
                    assert store - (ext + (ncol * nz if place == 0 else 0)) < 4    # nothing wasted beyond the alignment
                    # ... and without the store: every other offset as with it up to the store, the table where the store was, the end 'size' less (up to the alignment)
                    off0, _ = _plan(lib, B, nx, ny, nz, place, tallies, volume, table, 0)
                    assert off0[:9] == out[:9] and off0[11] == out[11], (off0, out)
                    assert 0 <= (end - off0[10]) - size < 4 and off0[9] == off0[12] <= store, (off0, out)
                    # the older entry point answers what it always did
                    old = np.zeros(12, np.int32)
                    q = np.array([nx, ny, nz, 1, 0, tallies, 0, 0, (nx + 3) // 4, 2, 0, 0, place, 0, waves, table, volume], np.int32)
                    assert lib.i3rc_hip_lds_plan(q.ctypes.data_as(B.ip), old.ctypes.data_as(B.ip)) == 0
                    assert [int(v) for v in old] == off0[:12]
    # too short arrays are refused
    q, out = np.zeros(16, np.int32), np.zeros(13, np.int32)
    assert lib.i3rc_hip_lds_plan_words(q.ctypes.data_as(B.ip), 16, out.ctypes.data_as(B.ip), 13) == 1
