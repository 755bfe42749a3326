"""Every single-GPU workload bench.py times, at the size it times it (50 M points, 4096^2), through the bench's own
--dump-outputs: the bands of the timed step -- pre-created chunk of pipelines on one scratch arena, the auto path choice,
device-resident results -- against the oracle on the same seeded cloud.  Point workloads: every dumped cell against the
oracle over the whole cloud.  Glyph workloads: the dumped cells inside four windows (an interior one across the LDS-tile
grid the line reports, the corner at (0, 0), a right-edge and the bottom-right corner window) against
tests/window_oracle.py.  Bars: Count / Max / Min bit-exact; Point Sum / Average 1e-5 of the double-accumulated oracle (+ 1e-6
absolute); glyph bands 1e-4 of it with a floor of 1e-3; NaN masks exact against the single-accumulated oracle."""
import importlib.util
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import pcr_oracle_py as O
import window_oracle as WO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, N = 4096, 50_000_000
MIN_SAMPLED = 2000

# scatter_path the auto choice takes for each workload at this size (gauss1.8 / gauss2 from a first run:
# sigma = 1.8 paints its 13 x 13 footprints in LDS tiles, sigma = 2 goes through moments): a change of the chooser shows up
# here by name
AUTO_PATH = {"C2": "binned", "point_avg": "binned", "C4": "binned", "gauss1": "binned", "gauss1.8": "binned",
             "gauss2": "moments", "gauss4": "moments", "gauss16": "moments", "line16": "binned"}
POINT_RTYPES = {"Sum": O.SUM, "Count": O.COUNT, "Average": O.AVERAGE, "Max": O.MAX, "Min": O.MIN}


def _load_bench():
    spec = importlib.util.spec_from_file_location("bench_parity_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BENCH = _load_bench()


def _bench(extra, d):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
           "--dump-outputs", str(d)] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def load_dump(d, prefix=""):
    """[(name, values with NaN where the _valid mask is 0)] in band order."""
    names = sorted(f for f in os.listdir(d) if f.startswith(prefix + "band") and f.endswith(".npy")
                   and not f.endswith("_valid.npy"))
    out = []
    for f in names:
        a, ok = np.load(os.path.join(d, f)), np.load(os.path.join(d, f[:-4] + "_valid.npy"))
        assert a.dtype == ok.dtype == np.float32 and a.shape == ok.shape and np.isin(ok, (0.0, 1.0)).all(), f
        out.append((f[len(prefix):-4].split("_", 1)[1], np.where(ok == 1, a, np.float32("nan"))))
    return out


def sample_index(cells, bands, world=1):
    """bench.dump_outputs' seeded sample of a strip of `cells` cells (None: the whole strip was written)."""
    k = min(cells, BENCH.DUMP_BYTES // (2 * 4 * bands * world))
    return None if k == cells else np.sort(np.random.default_rng(BENCH.DUMP_SEED).choice(cells, k, replace=False))


_CLOUDS = {}


def _cloud(wl):
    """bench.make_points(W, n, G, 0, G, seed=42) -- x, y, value are the same for every uniform workload, the Line's direction
    is drawn after them."""
    kind = "C4" if wl == "C4" else "line16"
    if kind not in _CLOUDS:
        _CLOUDS.clear()                                             # one 50 M-point cloud on the host at a time
        _CLOUDS[kind] = BENCH.make_points(kind, N, G, 0.0, float(G), seed=42)
    return _CLOUDS[kind]


def _grid():
    return O.make_grid((0.0, 0.0, float(G), float(G)))


def oracle_glyph(wl):
    _, glyph, arg, _ = BENCH.WORKLOADS[wl]
    if glyph == "gauss":
        max_r = 12.0 if arg == 4.0 else min(4.0 * arg, 64.0)          # bench.py make_specs
        return O.make_glyph(O.GLYPH_GAUSSIAN, sigma_x=arg, sigma_y=arg, max_radius=max_r)
    return O.make_glyph(O.GLYPH_LINE, half_length=arg, max_radius=arg + 2.0)


def check_cells(got, exact, single, rtol, floor, what, where=None):
    """got / exact / single: the same cells (1-D).  NaN mask exact against the single-accumulated oracle; values within
    rtol * max(floor, |exact|) of the double-accumulated one (rtol = 0: bit-exact against the single one).  -> (max rel err,
    cells compared).  where: (row, col) of every cell, for the messages."""
    def at(i):
        return f"cell {tuple(int(a) for a in where[i])}" if where is not None else f"sample {i}"

    gn, wn = np.isnan(got), np.isnan(single)
    bad = np.nonzero(gn != wn)[0]
    assert not len(bad), f"{what}: NaN mask differs from the oracle at {len(bad)} cells, first at {at(bad[0])}"
    assert np.array_equal(np.isnan(exact), wn), f"{what}: the oracle's two forms disagree on the NaN mask"
    keep = np.nonzero(~gn)[0]
    g, e, s = got[keep].astype(np.float64), exact[keep].astype(np.float64), single[keep]
    if rtol == 0.0:
        bad = np.nonzero(got[keep] != s)[0]
        assert not len(bad), f"{what}: {len(bad)} cells differ, first at {at(keep[bad[0]])}: {g[bad[0]]} vs {s[bad[0]]}"
        return 0.0, int(g.size)
    err = np.abs(g - e)
    lim = rtol * np.maximum(floor, np.abs(e)) if floor else rtol * np.abs(e) + 1e-6
    bad = np.nonzero(err > lim)[0]
    rel = float(np.max(err / np.maximum(np.abs(e), 1e-30))) if err.size else 0.0
    assert not len(bad), (f"{what}: {len(bad)} of {g.size} cells beyond the bar, first at {at(keep[bad[0]])}: got {g[bad[0]]} "
                          f"want {e[bad[0]]} (max rel {rel:.3g})")
    return rel, int(g.size)


def glyph_windows(lds_tile, s):
    """(name, (r0, r1, c0, c1)) of side s: one interior window whose edges lie inside LDS tiles and which crosses their
    grid in both directions, the grid corner at (0, 0) (the cloud starts 2 cells in: footprints clipped at the boundary),
    one on the right edge and the bottom-right corner (the LDS tiles of the largest index).  The direct path has no LDS
    tiles (the line reports 0 x 0)."""
    tw, th = lds_tile if all(lds_tile) else (1, 1)
    c0 = (2000 // tw) * tw - s // 2 + 1
    r0 = (2000 // th) * th - s // 2 + 1
    return [("interior", (r0, r0 + s, c0, c0 + s)), ("corner00", (0, s, 0, s)),
            ("right_edge", (G // 2 - s // 2, G // 2 + s // 2, G - s, G)), ("corner_br", (G - s, G, G - s, G))]


def check_glyph_dump(wl, d, line, report):
    x, y, v, ch = _cloud(wl)
    chans = {"direction": ch["direction"]} if BENCH.WORKLOADS[wl][1] == "line" else {}
    dump = load_dump(d)
    assert len(dump) == 1, [n for n, _ in dump]
    band = dump[0][1]
    idx = sample_index(G * G, 1)
    rows, cols = idx // G, idx % G
    s = 80 if WO.reach(_grid(), oracle_glyph(wl)) > 24 else 96        # sigma = 16: a smaller window, 9 409-cell footprints
    wins = glyph_windows(line["config"]["lds_tile"], s)
    glyph = oracle_glyph(wl)
    with ThreadPoolExecutor(len(wins)) as ex:
        wants = list(ex.map(lambda w: WO.window(_grid(), O.WEIGHTED_AVERAGE, x, y, v, w[1], glyph=glyph, **chans), wins))
    for (name, (r0, r1, c0, c1)), (exact, single) in zip(wins, wants):
        inside = np.nonzero((rows >= r0) & (rows < r1) & (cols >= c0) & (cols < c1))[0]
        assert len(inside) >= MIN_SAMPLED, (name, len(inside))
        rr, cc = rows[inside] - r0, cols[inside] - c0
        what = f"{wl} {line['config']['scatter_path']} window {name} {(r0, r1, c0, c1)}"
        rel, n = check_cells(band[inside], exact[rr, cc], single[rr, cc], 1e-4, 1e-3, what,
                             where=np.stack([rows[inside], cols[inside]], 1))
        report.append((wl, line["config"]["scatter_path"], name, rel, n))


def check_point_dump(wl, d, line, report):
    x, y, v, _ = _cloud(wl)
    og = _grid()
    dump = load_dump(d)
    names = list(BENCH.WORKLOADS[wl][2])                              # the bands in the order of the pipeline's reductions
    assert len(dump) == len(names), [n for n, _ in dump]
    idx = sample_index(G * G, len(dump))
    jobs = [(POINT_RTYPES[n], wide) for n in names for wide in (True, False)]
    with ThreadPoolExecutor(len(jobs)) as ex:
        runs = list(ex.map(lambda j: O.run(og, j[0], x, y, v, wide=j[1]), jobs))
    for b, ((_, got), name) in enumerate(zip(dump, names)):
        exact, single = (r.reshape(-1) if idx is None else r.reshape(-1)[idx] for r in runs[2 * b: 2 * b + 2])
        got = got.reshape(-1)
        assert got.shape == exact.shape
        rtol = 1e-5 if name in ("Sum", "Average") else 0.0
        rel, n = check_cells(got, exact, single, rtol, 0.0, f"{wl} band {b} {name}")
        report.append((wl, line["config"]["scatter_path"], f"all sampled cells, {name}", rel, n))


REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _print_report():
    yield
    if REPORT:
        print("\nworkload | path | window | max rel err vs f64 oracle | cells")
        for r in REPORT:
            print(f"{r[0]} | {r[1]} | {r[2]} | {r[3]:.3g} | {r[4]}")


@pytest.mark.parametrize("wl", list(AUTO_PATH))
def test_bench_workload_dump_matches_the_oracle(wl, tmp_path):
    line = _bench(["--workload", wl], tmp_path)
    c = line["config"]
    assert c["points_per_gpu"] == N and c["grid"] == f"{G}x{G}" and c["result"] == "device-resident"
    if BENCH.WORKLOADS[wl][1] == "point":
        check_point_dump(wl, tmp_path, line, REPORT)
    else:
        check_glyph_dump(wl, tmp_path, line, REPORT)
    assert c["scatter_path"] == AUTO_PATH[wl], f"{wl}: the auto choice is now {c['scatter_path']}, was {AUTO_PATH[wl]}"


@pytest.mark.parametrize("wl,path", [("gauss4", "moments"), ("gauss4", "binned"), ("gauss4", "direct"),
                                     ("line16", "binned"), ("line16", "direct")])
def test_bench_forced_path_dump_matches_the_oracle(wl, path, tmp_path):
    line = _bench(["--workload", wl, "--path", path], tmp_path)
    assert line["config"]["scatter_path"] == path
    check_glyph_dump(wl, tmp_path, line, REPORT)


def test_bench_host_cloud_host_result_leg_matches_the_oracle(tmp_path):
    """The drop-in leg reference scripts take: a host-resident cloud in, host-resident bands out (PCIe inside the step)."""
    line = _bench(["--workload", "gauss4", "--host-cloud", "--host-result"], tmp_path)
    c = line["config"]
    assert c["input"].startswith("host-resident") and c["result"].startswith("host")
    assert c["scatter_path"] == AUTO_PATH["gauss4"]
    check_glyph_dump("gauss4", tmp_path, line, REPORT)
