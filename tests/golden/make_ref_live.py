#!/usr/bin/env python3
"""Runs the REFERENCE's own CPU code (oracle/_ref/libpcr_ref.so, built by `make -C oracle ref`) on the inputs of the
test_*_live tests and stores what it returned: tests/golden/ref_live.npz.  Without oracle/_ref those tests compare the
oracle and the product against these recorded outputs instead of skipping; with it they also check that the recording
is still what the reference returns.

  merge/<rt>             pcr_ref_merge_state on merge_inputs() (raw state floats after the merge)
  probe/<i>              pcr_ref_accumulate_glyph on known-answer glyph case i (the raw state band)
  random/<seed>          "refused", or the digests (cases.digest) of the raw state and the finalized tile of
                         cases.random_glyph_case(seed), seeds 0..319
  lattice/<glyph>/<rt>   the digest of the raw state of pcr_ref_accumulate_glyph over the one tile of a 64 x 48 grid of
                         0.1-unit cells, on the cloud that sits on its cell edges (tests/routing_lattice.py "ref_tile"):
                         where the reference places a footprint whose centre is within an ulp of an edge
  tile_state/*           the .pcrt bytes the reference writes for tile_state_inputs(), what its reader returns for them,
                         and its file name for TILE_NAME_ARGS

Only runnable where oracle/_ref was built.  The fixture holds DATA only; inputs are regenerated from seeds.
"""
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import pcr_oracle_py as O   # noqa: E402
import cases                 # noqa: E402
import make_ref_vectors as MRV   # noqa: E402
import routing_lattice as RL     # noqa: E402

PATH = os.path.join(HERE, "ref_live.npz")
RANDOM_SEEDS = range(320)
TILE_NAME_ARGS = ("/a/b", 12, 345)
TILE_HEADER = (4, 5, 9, 7, 1, 1)          # row, col, width, height, floats per cell, reduction type (Max)
LATTICE_GLYPHS = {"gauss_r3": dict(type=cases.GAUSSIAN, sigma_x=0.1, sigma_y=0.1, max_radius=3.0),
                  "line": dict(type=cases.LINE, direction=0.6, half_length=0.35, max_radius=32.0)}
LATTICE_RTYPES = {"Sum": cases.SUM, "Count": cases.COUNT}


def merge_inputs(L):
    """(rt, a, b) for the six reduction types: two random raw states of 64 cells each, drawn in this order from seed 3."""
    rng = np.random.default_rng(3)
    for rt in range(6):
        k = L.pcro_state_floats(rt)
        a = rng.normal(size=k * 64).astype(np.float32)
        b = rng.normal(size=k * 64).astype(np.float32)
        yield rt, a, b


def probe_band(acc_fn, c):
    """Known-answer glyph case c accumulated by acc_fn over the whole grid: the raw state band [rows, cols], or None for a
    case whose tile is narrower than the grid (tile clipping needs the router)."""
    gj, s = c["grid"], c["spec"]
    if gj["tile"][0] < gj["dims"][0]:
        return None
    grid = O.make_grid(tuple(gj["bounds"]), cell=tuple(gj["cell"]), dims=tuple(gj["dims"]))
    rt = {"Sum": O.SUM, "Count": O.COUNT, "WeightedAverage": O.WEIGHTED_AVERAGE}[s["type"]]
    if s["glyph"] == "Gaussian":
        gl = O.make_glyph(O.GLYPH_GAUSSIAN, sigma_x=s["sigma"], sigma_y=s["sigma"], max_radius=s["max_radius"])
    else:
        gl = O.make_glyph(O.GLYPH_LINE, direction=s["direction"], half_length=s["half_length"], max_radius=s["max_radius"])
    pts, keep = O.make_points(c["x"], c["y"], c["value"])
    cells = grid.width * grid.height
    st = np.zeros(cells, dtype=np.float32)
    assert acc_fn(C.byref(gl), rt, C.byref(pts), st.ctypes.data, cells, C.byref(grid), 0, 0, grid.width, grid.height) == 0
    del keep
    return st.reshape(grid.height, grid.width)


def random_case_record(R, case):
    """("refused",) when the reference refuses the call, else (digest of the raw state, digest of the finalized tile)."""
    try:
        st, fin = MRV.run_glyph(R.pcr_ref_accumulate_glyph, R.pcr_ref_init_state, R.pcr_ref_finalize_state, case)
    except AssertionError:
        return ("refused",)
    return (cases.digest(st), cases.digest(fin))


def lattice_state(acc_fn, glyph, rt):
    """LATTICE_GLYPHS[glyph] accumulated by acc_fn over the whole "ref_tile" grid on its lattice cloud (the points inside the
    bounds, as a TileBatch would hold them): the raw state [rows, cols]."""
    grid = RL.grid("ref_tile")
    x, y, v = RL.cloud("ref_tile")
    ok = RL.in_bounds(grid, x, y)
    gl = O.make_glyph(**LATTICE_GLYPHS[glyph])
    pts, keep = O.make_points(x[ok], y[ok], v[ok])
    cells = grid.width * grid.height
    st = np.zeros(cells, dtype=np.float32)
    assert acc_fn(C.byref(gl), rt, C.byref(pts), st.ctypes.data, cells, C.byref(grid), 0, 0, grid.width, grid.height) == 0
    del keep
    return st.reshape(grid.height, grid.width)


def tile_state_inputs():
    return np.random.default_rng(2).normal(size=(1, 7, 9)).astype(np.float32)


def ref_tile_state(R, directory):
    """The reference writes tile_state_inputs() under TILE_HEADER and reads the file back: (bytes, header, data)."""
    R.pcr_ref_write_tile_state.argtypes = [C.c_char_p] + [C.c_int] * 6 + [C.c_void_p]
    R.pcr_ref_read_tile_state.argtypes = [C.c_char_p] + [C.POINTER(C.c_int)] * 6 + [C.c_void_p]
    st = tile_state_inputs()
    path = os.path.join(directory, "theirs.pcrt")
    assert R.pcr_ref_write_tile_state(path.encode(), *TILE_HEADER, st.ctypes.data) == 0
    v = [C.c_int(0) for _ in range(6)]
    out = np.zeros_like(st)
    assert R.pcr_ref_read_tile_state(path.encode(), *[C.byref(a) for a in v], out.ctypes.data) == 0
    return open(path, "rb").read(), [a.value for a in v], out


def ref_tile_name(R):
    buf = C.create_string_buffer(256)
    R.pcr_ref_tile_state_filename(TILE_NAME_ARGS[0].encode(), TILE_NAME_ARGS[1], TILE_NAME_ARGS[2], buf, 256)
    return buf.value.decode()


def main():
    R, L = O.ref_lib(), O.lib()
    if R is None:
        sys.exit("oracle/_ref/libpcr_ref.so not built (run: make -C oracle ref)")
    out = {}
    for rt, a, b in merge_inputs(L):
        assert R.pcr_ref_merge_state(rt, a.ctypes.data, b.ctypes.data, 64) == 0
        out[f"merge/{rt}"] = a
    with open(os.path.join(HERE, "reference_known_answers.json")) as f:
        known = json.load(f)
    for i, c in enumerate(known["glyph"]):
        band = probe_band(R.pcr_ref_accumulate_glyph, c)
        if band is not None:
            out[f"probe/{i}"] = band
    for seed in RANDOM_SEEDS:
        out[f"random/{seed}"] = np.array(random_case_record(R, cases.random_glyph_case(seed)))
    for glyph in LATTICE_GLYPHS:
        for name, rt in LATTICE_RTYPES.items():
            out[f"lattice/{glyph}/{name}"] = np.array(cases.digest(lattice_state(R.pcr_ref_accumulate_glyph, glyph, rt)))
    with tempfile.TemporaryDirectory() as d:
        data, header, back = ref_tile_state(R, d)
    out["tile_state/bytes"] = np.frombuffer(data, dtype=np.uint8)
    out["tile_state/read_header"] = np.array(header, dtype=np.int32)
    out["tile_state/read_data"] = back
    out["tile_state/filename"] = np.array(ref_tile_name(R))
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
