"""bench.py on one GPU as the driver runs it: a plain run prints the headline alone, --steps is the number of timed steps
(here more than one chunk of pre-created pipelines), and --dump-outputs writes the finalized bands of the last timed step --
whole, or as the fixed, seeded sample of cells when they exceed the budget -- which must be what the oracle computes from
the same seeded cloud."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pcr_oracle_py as O
from conftest import assert_band_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_bench():
    spec = importlib.util.spec_from_file_location("bench_single_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bench(extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + extra,
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def _want(bench, n, G):
    x, y, v, _ = bench.make_points("C2", n, G, 0.0, float(G), seed=42)
    og = O.make_grid((0.0, 0.0, float(G), float(G)))
    return [O.run(og, rt, x, y, v) for rt in (O.SUM, O.COUNT, O.AVERAGE)]


def _dumped(d):
    """The bands of a dump, no-data cells back as NaN: every file is finite float32, a band's _valid mask is 0 / 1 and
    its values are 0 where the mask is 0."""
    files = sorted(os.listdir(d))
    names = sorted(f for f in files if not f.endswith("_valid.npy"))
    assert [f.split("_")[0] for f in names] == ["band0", "band1", "band2"], files
    assert files == sorted(names + [f[:-4] + "_valid.npy" for f in names]), files
    assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 << 20
    bands = []
    for f in names:
        a, ok = np.load(os.path.join(d, f)), np.load(os.path.join(d, f[:-4] + "_valid.npy"))
        assert a.dtype == ok.dtype == np.float32 and a.shape == ok.shape
        assert np.isfinite(a).all() and np.isin(ok, (0.0, 1.0)).all() and (a[ok == 0] == 0).all(), f
        bands.append(np.where(ok == 1, a, np.float32("nan")))
    assert (bands[1] != bands[1]).any(), "the Count band should hold empty cells"
    return bands


def test_plain_run_is_the_headline_and_times_every_step(tmp_path):
    bench = _load_bench()
    n, G, steps = 200_000, 512, 2 * bench.TIMED_CHUNK + 7
    d = tmp_path / "out"
    r = _bench(["--steps", str(steps), "--warmup", "2", "--points", str(n), "--grid", str(G), "--dump-outputs", str(d)])
    assert r["steps"] == steps and r["warmup"] == 2 and r["n_gpus"] == 1
    assert r["metric"] == "Mpts/s ingest->finalize" and r["unit"] == "Mpts/s" and r["higher_is_better"] is True
    assert r["dtype"] == "f32" and r["ms_per_step"] > 0
    assert r["value"] == pytest.approx(n / r["ms_per_step"] / 1e3, rel=1e-2)
    for key in ("per_glyph", "e2e_host", "cpu_baseline", "gauss16_over_point", "selfcheck"):
        assert key not in r, key
    assert "measured_copy_GBps" not in r.get("roofline", {})
    got = _dumped(d)                                   # 3 x 1 MB: whole bands
    for b, (g, w) in enumerate(zip(got, _want(bench, n, G))):
        assert g.shape == (G, G)
        assert_band_close(g, w, *((0.0, 0.0) if b == 1 else (1e-5, 1e-6)), what=f"band {b}")


def test_dump_of_bands_over_the_budget_is_the_seeded_sample(tmp_path):
    bench = _load_bench()
    n, G = 1_000_000, 4096
    d = tmp_path / "out"
    _bench(["--steps", "2", "--warmup", "1", "--points", str(n), "--grid", str(G), "--dump-outputs", str(d)])
    got = _dumped(d)                                   # 3 x 64 MB (+ masks): sampled
    k = bench.DUMP_BYTES // (2 * 4 * 3)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(G * G, k, replace=False))
    for b, (g, w) in enumerate(zip(got, _want(bench, n, G))):
        assert g.shape == (k,)
        assert_band_close(g, w.reshape(-1)[idx], *((0.0, 0.0) if b == 1 else (1e-5, 1e-6)), what=f"band {b}")
