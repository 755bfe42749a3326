"""fill_nodata without a GPU: the host fill against the NumPy model of the contract (tests/fill_nodata_common.py) bit for bit,
the named properties of the contract, the thread count, the argument errors of pcr_hip_fill_nodata, the host-engine pipeline's
fill_nodata_radius (result, GeoTIFF, overview level), the create errors, and the host loop under ASan + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fill_nodata_common as F
import overviews_common as M
import pcr
from conftest import ROOT, load_cabi

PKG = os.path.join(ROOT, "pointcloud-raster_amd")
SHAPES = [(1, 1), (1, 40), (3, 5), (67, 129), (200, 150)]                 # (cols, rows)
RADII = [1, 2, 7, 32]


def host_fill(a, R, bands=None):
    return F.grid_bands(pcr.fill_nodata(F.make_grid([a]), R, bands))[0]


# ---- the arithmetic -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nan_fraction", [0.0, 0.2, 0.9, 1.0])
@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("shape", SHAPES)
def test_host_fill_equals_the_model(shape, R, nan_fraction):
    w, h = shape
    a = F.values(w, h, seed=w * 1000 + h + R, nan_fraction=nan_fraction)
    got = host_fill(a, R)
    F.bits_equal(got, F.fill(a, R), f"{w}x{h} R={R} nan={nan_fraction}")
    keep = ~np.isnan(a)
    F.bits_equal(got[keep], a[keep], "cells that are not NaN are copied")
    if nan_fraction == 1.0:
        F.bits_equal(got, a, "nothing valid anywhere: the source, payloads included")
    if nan_fraction == 0.0:
        F.bits_equal(got, a, "no hole: a copy")


@pytest.mark.parametrize("R", [1, 3, 6])
def test_radius_disc_keeps_the_core_of_a_wide_void(R):
    n = 2 * R + 3                                                          # the void's diameter
    W = H = n + 2 * (R + 2)
    a = F.finite_values(W, H, seed=R)
    yy, xx = np.mgrid[0:H, 0:W]
    cy = cx = W // 2
    void = (yy - cy) ** 2 + (xx - cx) ** 2 <= (n // 2) ** 2
    src = F.punch(a, void, seed=1)
    got = host_fill(src, R)
    # a void cell stays NaN exactly when no cell outside the void lies within R of it: computed from the geometry alone
    core = np.zeros_like(void)
    for r, c in np.argwhere(void):
        d2 = (yy - r) ** 2 + (xx - c) ** 2
        core[r, c] = not (~void & (d2 <= R * R)).any()
    assert core.any() and not core.all()
    assert (np.isnan(got) == core).all()
    F.bits_equal(got[core], src[core], "the core keeps its NaNs bit for bit")
    F.bits_equal(got, F.fill(src, R), "model")


def test_source_nan_payloads_survive_where_nothing_is_in_range():
    a = np.full((9, 11), 5.0, np.float32)
    a.view(np.uint32)[:, :7] = np.resize(F.NAN_PAYLOADS, (9, 7))           # a void 7 wide; R = 2 reaches two columns in
    got = host_fill(a, 2)
    F.bits_equal(got[:, :5], a[:, :5], "t == 0: the source NaN with its payload")
    assert (got[:, 5:] == 5.0).all()


def test_inf_neighbours():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    a = np.array([[inf, nan, -inf, nan, inf, nan, nan, nan, 2.0]], np.float32)
    got = host_fill(a, 1)
    assert got.view(np.uint32)[0, 1] == 0x7FC00000                        # Inf + -Inf: the one NaN, not the machine's
    assert got.view(np.uint32)[0, 3] == 0x7FC00000
    assert got[0, 5] == inf and np.isnan(got[0, 6]) and got[0, 7] == 2.0   # Inf is a value; out of range; an ordinary fill
    F.bits_equal(got, F.fill(a, 1), "model")
    den = np.array([[0x00000001, 0x7FC00000, 0x80000003]], np.uint32).view(np.float32)   # denormals are values: (1 - 3) / 2 units
    F.bits_equal(host_fill(den, 1), F.fill(den, 1), "denormals")
    assert host_fill(den, 1).view(np.uint32)[0, 1] == 0x80000001


def test_bands_argument():
    arrays = [F.values(40, 30, seed=s, nan_fraction=0.3) for s in (1, 2, 3)]
    g = F.make_grid(arrays, ["mean", "count <n>", "max"])
    for bands in (None, [0, 2], [1]):
        out = pcr.fill_nodata(g, 3, bands)
        assert out.location() == pcr.MemoryLocation.Host and (out.cols(), out.rows()) == (40, 30)
        for b in range(3):
            assert out.band_desc(b).name == g.band_desc(b).name
            want = F.fill(arrays[b], 3) if bands is None or b in bands else arrays[b]
            F.bits_equal(F.grid_bands(out)[b], want, f"bands={bands} band {b}")
        for b in range(3):
            F.bits_equal(F.grid_bands(g)[b], arrays[b], "the source grid is only read")
    for R in (0, 33, -1):
        with pytest.raises(RuntimeError, match="radius must be between 1 and 32"):
            pcr.fill_nodata(g, R)
    with pytest.raises(RuntimeError, match="band index outside"):
        pcr.fill_nodata(g, 1, [3])


THREADS_SCRIPT = """
import sys
sys.path[:0] = {paths!r}
import numpy as np
import fill_nodata_common as F
import pcr
a = F.values(150, 120, seed=9, nan_fraction=0.4)
out = F.grid_bands(pcr.fill_nodata(F.make_grid([a]), 5))[0]
sys.stdout.write(out.tobytes().hex())
"""


def test_thread_count_does_not_change_the_bits():
    paths = [os.path.join(ROOT, "tests"), os.path.dirname(os.path.dirname(pcr.__file__))]
    runs = []
    for n in ("1", "4"):
        env = dict(os.environ, OMP_NUM_THREADS=n)
        out = subprocess.run([sys.executable, "-c", THREADS_SCRIPT.format(paths=paths)], capture_output=True, text=True, env=env,
                             timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        runs.append(out.stdout)
    assert len(runs[0]) == 150 * 120 * 8 and runs[0] == runs[1]
    a = F.values(150, 120, seed=9, nan_fraction=0.4)
    assert runs[0] == F.fill(a, 5).tobytes().hex()


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------
def test_fill_nodata_argument_errors_need_no_gpu():
    A = load_cabi()
    L = A.lib()
    src, dst = C.c_void_p(0x100000), C.c_void_p(0x200000)       # never dereferenced: every call below is refused before any HIP call
    def call(s=src, d=dst, w=16, h=16, ss=16, ds=16, R=4):
        return L.pcr_hip_fill_nodata(s, d, w, h, ss, ds, R, None)
    for kw, msg in ((dict(s=None), b"null argument"), (dict(d=None), b"null argument"),
                    (dict(w=0), b"must be positive"), (dict(h=-1), b"must be positive"),
                    (dict(ss=15), b"src_stride smaller than width"), (dict(ds=15), b"dst_stride smaller than width"),
                    (dict(R=0), b"radius must be between 1 and 32"), (dict(R=33), b"radius must be between 1 and 32"),
                    (dict(d=src), b"dst overlaps src"),
                    (dict(d=C.c_void_p(0x100000 + 4 * (15 * 16 + 15))), b"dst overlaps src"),      # the last cell of src
                    (dict(s=C.c_void_p(0x200000 + 4 * 20), ss=64), b"dst overlaps src")):
        assert call(**kw) == 1, kw
        assert msg in L.pcr_hip_last_error(), (kw, L.pcr_hip_last_error())
    assert L.pcr_hip_abi_version() == 5


def test_symbol_table_still_equals_the_header():
    A = load_cabi()
    text = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    assert "pcr_hip_fill_nodata" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(pcr_hip_[a-z0-9_]+)\s*\(", text)))
    assert sorted(A.SYMBOLS) == names and "pcr_hip_fill_nodata" in names
    assert hasattr(C.CDLL(A.LIB_PATH), "pcr_hip_fill_nodata")


# ---- the host-engine pipeline ---------------------------------------------------------------------------------------------
W, H, NPTS, RADIUS = 64, 48, 600, 3


@pytest.fixture(scope="module")
def host_case():
    pts = F.cloud(W, H, NPTS, seed=71)
    pipe = pcr.Pipeline.create(F.pipeline_cfg(W, H, pcr.ExecutionMode.CPU))
    assert pipe is not None, pcr.pipeline_create_error()
    pipe.ingest(pts)
    pipe.finalize()
    raw = F.grid_bands(pipe.result())
    assert np.isnan(raw[0]).any() and not np.isnan(raw[0]).all()
    return pts, raw, F.expect_filled(raw, RADIUS)


def test_default_radius_is_zero_and_changes_nothing(host_case):
    pts, raw, _ = host_case
    assert pcr.PipelineConfig().fill_nodata_radius == 0
    pipe = pcr.Pipeline.create(F.pipeline_cfg(W, H, pcr.ExecutionMode.CPU, radius=0))
    pipe.ingest(pts)
    pipe.finalize()
    for b, got in enumerate(F.grid_bands(pipe.result())):
        F.bits_equal(got, raw[b], f"band {b}")


@pytest.mark.parametrize("cog", [False, True])
def test_host_pipeline_fills_average_and_max_not_count(tmp_path, host_case, cog):
    pts, raw, want = host_case
    cfg = F.pipeline_cfg(W, H, pcr.ExecutionMode.CPU, radius=RADIUS)
    cfg.output_path, cfg.write_cog = str(tmp_path / "f.tif"), cog
    pipe = pcr.Pipeline.create(cfg)
    assert pipe is not None, pcr.pipeline_create_error()
    assert pipe.engine() == "host"
    pipe.ingest(pts)
    pipe.finalize()
    got = F.grid_bands(pipe.result())
    for b in range(3):
        F.bits_equal(got[b], want[b], f"band {b}")
        F.bits_equal(pcr.read_geotiff_band(cfg.output_path, b), want[b], f"file band {b}")
    F.bits_equal(got[1], raw[1], "Count is untouched")
    assert np.isnan(raw[0]).sum() > np.isnan(got[0]).sum() > 0            # holes were filled; the empty strip keeps a NaN core
    pipe.finalize()                                                        # the state is untouched: the same again
    for b in range(3):
        F.bits_equal(F.grid_bands(pipe.result())[b], want[b], f"second finalize, band {b}")


def test_host_pipeline_overview_level_is_made_from_the_filled_band(tmp_path):
    # write_cog's rule gives a level only from 512 cells a side: a sparse cloud on such a grid
    Wc, Hc = 520, 512
    pts = F.cloud(Wc, Hc, 60_000, seed=72)
    pipe0 = pcr.Pipeline.create(F.pipeline_cfg(Wc, Hc, pcr.ExecutionMode.CPU))
    pipe0.ingest(pts)
    pipe0.finalize()
    raw = F.grid_bands(pipe0.result())
    want = F.expect_filled(raw, 2)
    cfg = F.pipeline_cfg(Wc, Hc, pcr.ExecutionMode.CPU, radius=2)
    cfg.output_path, cfg.write_cog = str(tmp_path / "c.tif"), True
    pipe = pcr.Pipeline.create(cfg)
    pipe.ingest(pts)
    pipe.finalize()
    assert pcr.read_geotiff_overviews(cfg.output_path) == [(260, 256)]
    for b in range(3):
        F.bits_equal(F.grid_bands(pipe.result())[b], want[b], f"band {b}")
        F.bits_equal(pcr.read_geotiff_band(cfg.output_path, b, 1), M.down(want[b]), f"band {b} level 1")
    assert np.isnan(raw[0]).sum() > np.isnan(want[0]).sum()


def test_create_errors():
    cfg = F.pipeline_cfg(W, H, pcr.ExecutionMode.CPU, radius=33)
    assert pcr.Pipeline.create(cfg) is None
    assert pcr.pipeline_create_error() == "pipeline: fill_nodata_radius must be between 0 and 32"
    cfg = F.pipeline_cfg(W, H, pcr.ExecutionMode.CPU, radius=-1)
    assert pcr.Pipeline.create(cfg) is None
    assert pcr.pipeline_create_error() == "pipeline: fill_nodata_radius must be between 0 and 32"
    for mode in (pcr.ExecutionMode.CPU, pcr.ExecutionMode.GPU):
        cfg = F.pipeline_cfg(W, H, mode, radius=3)
        cfg.shard_row_begin, cfg.shard_row_end = 16, 32
        assert pcr.Pipeline.create(cfg) is None
        assert pcr.pipeline_create_error() == ("pipeline: fill_nodata_radius needs the whole grid; "
                                               "fill the gathered grid with fill_nodata")


# ---- sanitizers (the host loop alone, in a program of its own) ----------------------------------------------------------------
def test_host_fill_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    host = os.path.join(PKG, "host")
    exe = str(tmp_path / "fill_nodata_san")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fopenmp", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=undefined,float-cast-overflow", "-fno-omit-frame-pointer",
                    "-I", os.path.join(host, "include"), "-I", os.path.join(host, "src"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "fill_nodata_san.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", OMP_NUM_THREADS="4")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "host fill survived" in out.stdout
