"""bench.py's --dump-outputs writer on the host: what it keeps of a step's results, and its 64 MB cap."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _results(big):
    from i3rc_monte_carlo_model_amd import binding as B

    rng = np.random.default_rng(7)
    return {"fluxUp": rng.random((4, 8), dtype=np.float32), "volumeAbsorption": rng.random(big, dtype=np.float32),
            "raw": np.zeros(16, np.float64), "counters": {k: float(i) for i, k in enumerate(B.COUNTER_NAMES)}}


def test_dump_writes_the_callers_arrays(tmp_path):
    from i3rc_monte_carlo_model_amd import binding as B

    res = _results((3, 4, 8))
    _bench_module().dump_outputs(str(tmp_path), res)
    assert sorted(os.listdir(str(tmp_path))) == ["counters.npy", "fluxUp.npy", "volumeAbsorption.npy"]
    up = np.load(str(tmp_path / "fluxUp.npy"))
    assert up.dtype == np.float32 and np.array_equal(up, res["fluxUp"])
    cnt = np.load(str(tmp_path / "counters.npy"))
    assert cnt.dtype == np.float64 and list(cnt) == [float(i) for i in range(len(B.COUNTER_NAMES))]


def test_dump_above_64_mb_is_a_fixed_sample(tmp_path):
    res = _results((20_000_000,))          # 80 MB of float32
    bench = _bench_module()
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res)
    sizes = {f: os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))}
    assert sum(sizes.values()) <= 64 << 20, sizes
    va = np.load(str(tmp_path / "a" / "volumeAbsorption.npy"))
    assert va.dtype == np.float32 and 0 < va.size < 20_000_000
    assert np.isin(va, res["volumeAbsorption"]).all()
    for f in sizes:
        assert np.array_equal(np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f))), f
