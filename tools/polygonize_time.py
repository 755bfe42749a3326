#!/usr/bin/env python3
"""What polygonize costs on the device (profiles/polygonize.md).  Prints one JSON line per case.

Two G x G float32 label bands in HBM (default 4096): the tree-id band pcr_hip_trees makes of tools/trees_time.py's canopy (a few
hundred thousand crowns), and a checkerboard of two zones over a background of no zone (every lattice corner a saddle, four
boundary edges per zone cell: the most edges a band can have).  The device's ring table is first compared with the host twin's,
every array.  Then the three calls are timed with device events between the phases -- pcr_hip_polygonize_edges; inside
pcr_hip_polygonize_rings the edge list, the key rounds, the rank rounds and the scan (pcr_hip_polygonize_params.events); and
pcr_hip_polygonize_fetch -- W warm-ups, then the MEDIAN of K runs.  Beside them what the calls replace on the same machine: the
device-to-host copy of the band plus the host twin (wall clock), and pcr_hip_copy_kernel over the bytes the cell pass reads.
`bytes` is what a phase reads and writes at least, `GB/s` that over its time.

    python tools/polygonize_time.py [--grid 4096] [--steps 5] [--warmup 1] [--md profiles/polygonize.md]

--md: also writes the tables as Markdown."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pointcloud-raster_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from pcr import _cabi as A  # noqa: E402

PHASES = ["cells + scan", "edge list", "key rounds", "rank rounds", "ring scan", "fetch"]


def tree_ids(L, G):
    from trees_time import band
    z = band(G)
    src = A.DeviceBuffer.from_numpy(z)
    d_id = A.DeviceBuffer(4 * G * G)
    nbytes = C.c_size_t(0)
    A.check(L.pcr_hip_trees_work_bytes(G, G, C.byref(nbytes)))
    work = A.DeviceBuffer(nbytes.value)
    p = A.TreeParams()
    A.check(L.pcr_hip_trees(src.ptr, G, G, G, C.byref(p), d_id.ptr, G, None, G, work.ptr, nbytes.value, None))
    A.check(L.pcr_hip_stream_synchronize(None))
    ids = d_id.to_numpy(np.float32, (G, G))
    for d in (src, d_id, work):
        d.free()
    return ids


def checkerboard(G):
    rr, cc = np.mgrid[0:G, 0:G]
    a = np.full((G, G), np.nan, np.float32)
    black = (rr + cc) % 2 == 0
    a[black] = 1 + (rr[black] // 2 + cc[black]) % 2
    return a


def host_twin(L, z):
    h, w = z.shape
    n = [C.c_int64(0) for _ in range(3)]
    A.check(L.pcr_hip_polygonize_host(z.ctypes.data, w, h, w, *[C.byref(x) for x in n], 0, 0, None, None, None, None))
    E, R, V = (x.value for x in n)
    t = [np.zeros(R, np.uint32), np.zeros(R + 1, np.int64), np.zeros(V, np.int32), np.zeros(V, np.int32)]
    t0 = time.perf_counter()
    A.check(L.pcr_hip_polygonize_host(z.ctypes.data, w, h, w, None, None, None, R, V, *[x.ctypes.data for x in t]))
    return E, t, (time.perf_counter() - t0) * 1e3


def case(L, name, z, steps, warmup):
    G = z.shape[0]
    band = A.DeviceBuffer.from_numpy(z)
    copy_dst = A.DeviceBuffer(4 * G * G)
    cb = C.c_size_t(0)
    A.check(L.pcr_hip_polygonize_cells_work_bytes(G, G, C.byref(cb)))
    cells = A.DeviceBuffer(cb.value)
    ev = [C.c_void_p() for _ in range(11)]
    for e in ev:
        A.check(L.pcr_hip_event_create(C.byref(e)))

    def ms(a, b):
        out = C.c_float(0.0)
        A.check(L.pcr_hip_event_elapsed_ms(ev[a], ev[b], C.byref(out)))
        return out.value

    E, R, V, kr, rr = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int(0), C.c_int(0)
    rings = table = None
    rb = C.c_size_t(0)
    times = {p: [] for p in PHASES}
    times["copy kernel"], times["whole (wall)"] = [], []
    for i in range(warmup + steps):
        A.check(L.pcr_hip_stream_synchronize(None))
        w0 = time.perf_counter()
        A.check(L.pcr_hip_event_record(ev[0], None))
        A.check(L.pcr_hip_polygonize_edges(band.ptr, G, G, G, cells.ptr, cb.value, None))
        A.check(L.pcr_hip_event_record(ev[1], None))
        A.check(L.pcr_hip_polygonize_count(cells.ptr, cb.value, C.byref(E), None, None, None, None, None))
        if rings is None:                                            # (E, R and V are the same in every run)
            A.check(L.pcr_hip_polygonize_rings_work_bytes(E.value, C.byref(rb)))
            rings = A.DeviceBuffer(rb.value)
        params = A.PolygonizeParams(events=[e.value for e in ev[3:7]])
        A.check(L.pcr_hip_event_record(ev[2], None))
        A.check(L.pcr_hip_polygonize_rings(band.ptr, G, G, G, cells.ptr, cb.value, E.value, rings.ptr, rb.value, C.byref(params), None))
        A.check(L.pcr_hip_polygonize_count(cells.ptr, cb.value, C.byref(E), C.byref(R), C.byref(V), C.byref(kr), C.byref(rr), None))
        if table is None:
            table = [A.DeviceBuffer(4 * R.value), A.DeviceBuffer(8 * (R.value + 1)), A.DeviceBuffer(4 * V.value), A.DeviceBuffer(4 * V.value)]
        A.check(L.pcr_hip_event_record(ev[7], None))
        A.check(L.pcr_hip_polygonize_fetch(band.ptr, G, G, G, cells.ptr, cb.value, E.value, rings.ptr, rb.value, R.value, V.value,
                                           *[t.ptr for t in table], None))
        A.check(L.pcr_hip_event_record(ev[8], None))
        A.check(L.pcr_hip_stream_synchronize(None))
        wall = (time.perf_counter() - w0) * 1e3
        A.check(L.pcr_hip_event_record(ev[10], None))
        A.check(L.pcr_hip_copy_kernel(copy_dst.ptr, band.ptr, 4 * G * G, 1, None))
        A.check(L.pcr_hip_event_record(ev[9], None))
        A.check(L.pcr_hip_stream_synchronize(None))
        if i < warmup:
            continue
        for p, (a, b) in zip(PHASES, ((0, 1), (2, 3), (3, 4), (4, 5), (5, 6), (7, 8))):
            times[p].append(ms(a, b))
        times["copy kernel"].append(ms(10, 9))
        times["whole (wall)"].append(wall)

    # ---- the table against the host twin, and what the calls replace
    t0 = time.perf_counter()
    back = band.to_numpy(np.float32, (G, G))
    d2h = (time.perf_counter() - t0) * 1e3
    hE, want, twin_ms = host_twin(L, back)
    assert hE == E.value and len(want[0]) == R.value and len(want[2]) == V.value, "counts differ from the host twin"
    for d, w_, nm in zip(table, want, ("ring_zone", "ring_offset", "vertex_row", "vertex_col")):
        assert np.array_equal(d.to_numpy(w_.dtype, w_.shape), w_), f"{nm} differs from the host twin"
    n, e = G * G, E.value
    # bytes: the band and its codes; per edge 4 + 4 + 1 + 8 written and the cell codes read; per working round 8 + 8 read, 8 written
    moved = [4 * n + 2 * n, 2 * n + 17 * e, 24 * e * kr.value, 24 * e * rr.value + 21 * e, 17 * e, 29 * e + 8 * V.value + 12 * R.value]
    med = {k: statistics.median(v) for k, v in times.items()}
    rows = [{"phase": p, "ms": round(med[p], 4), "MB": round(b / 1e6, 1), "GB_per_s": round(b / 1e6 / max(med[p], 1e-6), 1)}
            for p, b in zip(PHASES, moved)]
    out = {"case": name, "grid": G, "edges": e, "rings": R.value, "vertices": V.value, "zones": int(len(np.unique(want[0]))),
           "rounds_enqueued": math.ceil(math.log2(e)) + 1, "key_rounds_worked": kr.value, "rank_rounds_worked": rr.value,
           "device_ms": round(sum(med[p] for p in PHASES), 4), "whole_wall_ms": round(med["whole (wall)"], 4),
           "copy_kernel_ms": round(med["copy kernel"], 4), "d2h_ms": round(d2h, 3), "host_twin_ms": round(twin_ms, 3),
           "cells_work_MB": round(cb.value / 1e6, 1), "rings_work_MB": round(rb.value / 1e6, 1), "steps": steps, "warmup": warmup,
           "equals_host_twin": True, "phases": rows}
    for d in [band, copy_dst, cells, rings] + table:
        d.free()
    for e_ in ev:
        A.check(L.pcr_hip_event_destroy(e_))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    L = A.lib()
    if A.device_count() < 1:
        raise RuntimeError("no HIP device")
    G = args.grid
    results = [case(L, "tree ids", tree_ids(L, G), args.steps, args.warmup), case(L, "checkerboard", checkerboard(G), args.steps, args.warmup)]
    if args.md:
        with open(args.md, "w") as f:
            f.write(f"Polygonize on {G} x {G} label bands, the ring table equal to the host twin's, every array (tools/polygonize_time.py; "
                    f"median of {args.steps} runs after {args.warmup} warm-up; device events between the phases).\n")
            for r in results:
                f.write(f"\n**{r['case']}**: {r['zones']} zones, E = {r['edges']} boundary edges, R = {r['rings']} rings, V = {r['vertices']} "
                        f"vertices.  {r['rounds_enqueued']} rounds enqueued per doubling phase; {r['key_rounds_worked']} key rounds and "
                        f"{r['rank_rounds_worked']} rank rounds changed something.  Work areas {r['cells_work_MB']} MB (cells) and "
                        f"{r['rings_work_MB']} MB (rings).  Sum of the phases {r['device_ms']:.3f} ms; the three calls with their two "
                        f"waits, wall clock, {r['whole_wall_ms']:.3f} ms.  What they replace: the device-to-host copy of the band "
                        f"{r['d2h_ms']:.1f} ms plus the host twin {r['host_twin_ms']:.1f} ms.  pcr_hip_copy_kernel over the band's bytes: "
                        f"{r['copy_kernel_ms']:.3f} ms.\n\n")
                f.write("| phase | ms | MB read + written (at least) | GB/s |\n|---|---|---|---|\n")
                for p in r["phases"]:
                    f.write(f"| {p['phase']} | {p['ms']:.3f} | {p['MB']:.1f} | {p['GB_per_s']:.0f} |\n")


if __name__ == "__main__":
    main()
