"""bench.py's multi-rank line (C5: 16384 columns, row-block shards, halo reduce) against the oracle, through the per-rank
strip dumps of --dump-outputs.  Ranks share one GPU over gloo (tests/test_gpu_bench_multi.py explains why a one-GPU box
admits no more than four).  Each rank's cloud is regenerated in this process with bench.device_cloud_uniform and the bench's
own arguments, masked on the device by tests/window_oracle.py, and the sampled cells of every rank's strip are compared in
windows across the shard boundaries (the halo reduce), the reference-tile corners where Q4 clips footprints at the real size,
and -- at N = 2 -- the seams between the row bands the Gaussian's 16-byte front end sweeps a shard in."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import pcr_oracle_py as O
import window_oracle as WO
from test_gpu_bench_parity import BENCH, MIN_SAMPLED, check_cells, load_dump, sample_index

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B16_MAX_BINS = 16384            # tiles one pass of the 16-byte front end counts (csrc/bin16.hpp, b16::max_bins)
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _print_report():
    yield
    if REPORT:
        print("\nworkload | path | window | max rel err vs f64 oracle | cells")
        for r in REPORT:
            print(f"{r[0]} | {r[1]} | {r[2]} | {r[3]:.3g} | {r[4]}")


def _run(extra, ranks, d):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(ranks), "--steps", "1",
           "--warmup", "1", "--backend", "gloo", "--same-device", "--dump-outputs", str(d)] + extra
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def _selected(world, G, H, n, wins, margin, point):
    """Every rank's cloud as the bench generates it (device_cloud_uniform, seed 42 + rank, y-range of its row block),
    masked on the device: per window, the host arrays of the points (of all ranks) whose footprint can reach it."""
    import torch
    BENCH._imports()
    og = O.make_grid((0.0, 0.0, float(G), float(H)))
    out = [[] for _ in wins]
    for rank in range(world):
        r0, r1 = BENCH.row_block(rank, world, H)
        y_hi, y_lo = float(H - r0), float(H - r1)
        c = BENCH.device_cloud_uniform(n, 2.0, G - 2.0, y_lo + (2.0 if rank == world - 1 else 0.0),
                                       y_hi - (2.0 if rank == 0 else 0.0), seed=42 + rank)
        ptrs = c.device_ptrs()
        t = [torch.as_tensor(BENCH.pcr.DeviceArrayView(ptrs[k], (n,), ts, owner=c), device="cuda")
             for k, ts in (("x", "<f8"), ("y", "<f8"), ("value", "<f4"))]
        for k, w in enumerate(wins):
            m = WO.select(og, t[0], t[1], w, margin, point=point)
            out[k].append([a[m].cpu().numpy() for a in t])
            del m
        del t, c, ptrs
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    return og, [[np.concatenate([p[i] for p in per]) for i in range(3)] for per in out]


def _check(line, d, world, G, H, n, glyph, wins, tag):
    """wins: [(name, (r0, r1, c0, c1))].  Every rank's dumped sample inside each window against the oracle."""
    margin = WO.reach(O.make_grid((0.0, 0.0, float(G), float(H))), glyph)
    og, pts = _selected(world, G, H, n, [w for _, w in wins], margin, glyph is None)
    strips = []
    for rank in range(world):
        r0, r1 = BENCH.row_block(rank, world, H)
        dump = load_dump(d, prefix=f"rank{rank}_")
        assert len(dump) == 1, [a for a, _ in dump]
        idx = sample_index((r1 - r0) * G, 1, world)
        strips.append((r0 + idx // G, idx % G, dump[0][1]))
    for (name, w), (x, y, v) in zip(wins, pts):
        exact, single = WO.window(og, O.AVERAGE, x, y, v, w, glyph=glyph)
        wr0, wr1, wc0, wc1 = w
        total, worst = 0, 0.0
        for rank, (rows, cols, band) in enumerate(strips):
            inside = np.nonzero((rows >= wr0) & (rows < wr1) & (cols >= wc0) & (cols < wc1))[0]
            if not len(inside):
                continue
            rr, cc = rows[inside] - wr0, cols[inside] - wc0
            rel, k = check_cells(band[inside], exact[rr, cc], single[rr, cc], 1e-5 if glyph is None else 1e-4,
                                 0.0 if glyph is None else 1e-3, f"{tag} rank {rank} window {name} {w}",
                                 where=np.stack([rows[inside], cols[inside]], 1))
            total, worst = total + k, max(worst, rel)
        assert total >= MIN_SAMPLED, (name, total)
        REPORT.append((tag, line["config"]["scatter_path"], name, worst, total))


def band_seams(line, G, H, world):
    """The row bands the cell-tile Gaussian sweeps each rank's state window in (csrc/scatter_cells.hip, cells_gauss: as many
    tile rows per band as B16_MAX_BINS // tiles per row; state window = the owned rows + halo_rows on each side inside the
    grid), from the tile the line reports.  -> (rows of rank 0's bands, [(name, global seam row)] of every rank)."""
    BENCH._imports()                                                  # (row_block: after the bench's own processes)
    c = line["config"]
    tw, th = c["lds_tile"]
    halo = c["halo_rows"]
    bins_x = -(-G // tw)
    band_rows = (B16_MAX_BINS // bins_x) * th
    seams, bands0 = [], None
    for rank in range(world):
        r0, r1 = BENCH.row_block(rank, world, H)
        s0, s1 = max(0, r0 - halo), min(H, r1 + halo)
        if rank == 0:
            bands0 = [min(band_rows, s1 - s0 - b) for b in range(0, s1 - s0, band_rows)]
        seams += [(f"band_seam_rank{rank}_row{s}", s) for s in range(s0 + band_rows, s1, band_rows)]
    # the line (rank 0's) took the cell-tile path in these bands: its bin count is theirs
    assert c["scatter_path"] == "binned" and tw == 58, c
    assert c["num_bins"] == bins_x * sum(-(-b // th) for b in bands0), (c["num_bins"], c["lds_tile"], bands0)
    return bands0, seams


def _c5_windows(G):
    """Across the boundary of the two ranks' blocks, and around the reference-tile corners (4096, 4096) -- the first rows
    past 4096 of rank 0's 16384-wide shard -- and (12288, 12288) in rank 1's: 160 x 640 cells, ~2 400 sampled."""
    return [("shard_boundary", (G // 2 - 80, G // 2 + 80, 6000, 6640)),
            ("tile_corner_4096", (4096 - 80, 4096 + 80, 4096 - 320, 4096 + 320)),
            ("tile_corner_12288", (12288 - 80, 12288 + 80, 12288 - 320, 12288 + 320))]


@pytest.mark.parametrize("wl", ["C5_point", "C5_gauss1"])
def test_two_ranks_at_the_c5_size_match_the_oracle(wl, tmp_path):
    """N = 2 at the real C5 size: 8192-row blocks end on reference-tile boundaries (no footprint crosses them: Q4), and a
    Gaussian shard's 8196-row state window holds more 58 x 40 cell tiles than one pass of the 16-byte front end counts, so
    it is swept in row bands -- the seams between them are windows of their own."""
    G, n, world = 16384, 500_000_000, 2
    line = _run(["--workload", wl, "--grid", str(G), "--points", str(n)], world, tmp_path)
    c = line["config"]
    assert c["grid"] == f"{G}x{G}" and c["rows_per_gpu"] == G // 2 and c["points_total"] == world * n
    glyph, wins = None, _c5_windows(G)
    if wl == "C5_gauss1":
        glyph = O.make_glyph(O.GLYPH_GAUSSIAN, sigma_x=1.0, sigma_y=1.0, max_radius=4.0)
        assert c["halo_rows"] == 4 and c["tiles_local"] is True
        bands0, seams = band_seams(line, G, G, world)
        assert len(bands0) >= 2 and len(seams) >= 2 * (len(bands0) - 1), (bands0, seams)
        wins += [(name, (s - 80, s + 80, 5000, 5640)) for name, s in seams]
    _check(line, tmp_path, world, G, G, n, glyph, wins, f"{wl} N=2")


def test_four_ranks_of_the_eight_rank_geometry_match_the_oracle(tmp_path):
    """The 2048-row blocks of N = 8 as four ranks on 16384 x 8192: blocks 0|1 and 2|3 meet inside a reference tile (the halo
    reduce carries the footprints across), 1|2 on a tile boundary.  A 2056-row state window of 20-row cell tiles exceeds one
    binning pass, so the cell tiles are 40 rows tall and the window is one band."""
    G, H, n, world = 16384, 8192, 40_000_000, 4
    line = _run(["--workload", "C5_gauss1", "--grid", str(G), "--height", str(H), "--points", str(n)], world, tmp_path)
    c = line["config"]
    assert c["grid"] == f"{G}x{H}" and c["rows_per_gpu"] == 2048 and c["halo_rows"] == 4 and c["tiles_local"] is False
    bands0, _ = band_seams(line, G, H, world)
    assert c["lds_tile"] == [58, 40] and len(bands0) == 1, (c["lds_tile"], bands0)
    wins = [("shard_boundary_2048", (2048 - 48, 2048 + 48, 9000, 9512)),
            ("shard_boundary_6144", (6144 - 48, 6144 + 48, 9000, 9512)),
            ("tile_corner_4096", (4096 - 48, 4096 + 48, 4096 - 256, 4096 + 256))]
    glyph = O.make_glyph(O.GLYPH_GAUSSIAN, sigma_x=1.0, sigma_y=1.0, max_radius=4.0)
    _check(line, tmp_path, world, G, H, n, glyph, wins, "C5_gauss1 N=4 (16384x8192)")
