"""GeoTIFF overviews without a GPU: host build_overviews against the NumPy model of the contract (tests/overviews_common.py)
bit for bit, the level rule, the file (this build's reader, Pillow, and a walk over the directories), the host-side
pipelines' write_cog, and the argument errors of pcr_hip_downsample2."""
import ctypes as C
import struct

import numpy as np
import pytest

import overviews_common as M
import pcr
from conftest import load_cabi

MODES = ["average", "nearest"]
SHAPES = [(1, 1), (1, 7), (2, 2), (3, 5), (129, 65), (301, 203)]          # (cols, rows)


def grid_config(W, H, epsg=32618):
    c = pcr.GridConfig()
    c.bounds = pcr.BBox(500000.0, 4100000.0 - 2.0 * H, 500000.0 + 2.0 * W, 4100000.0)
    c.cell_size_x, c.cell_size_y = 2.0, -2.0
    c.compute_dimensions()
    assert (c.width, c.height) == (W, H)
    c.crs = pcr.CRS.from_epsg(epsg)
    return c


# ---- the arithmetic -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nan_fraction", [0.0, 0.2, 0.9, 1.0])
def test_host_levels_equal_the_model(shape, nan_fraction, mode):
    w, h = shape
    a = M.values(w, h, seed=w * 1000 + h, nan_fraction=nan_fraction)
    n = M.max_levels(w, h)
    levels = pcr.build_overviews(M.make_grid([a]), n, mode)
    assert len(levels) == n
    for k, (lv, want) in enumerate(zip(levels, M.pyramid(a, n, mode))):
        assert lv.location() == pcr.MemoryLocation.Host
        M.bits_equal(M.grid_bands(lv)[0], want, f"{w}x{h} {mode} level {k + 1}")
    if n:
        assert (levels[-1].cols(), levels[-1].rows()) == (1, 1)


@pytest.mark.parametrize("mode", MODES)
def test_three_bands_keep_their_descriptions(mode):
    arrays = [M.values(129, 65, seed=s) for s in (1, 2, 3)]
    g = M.make_grid(arrays, ["sum", "mean <m>", "count"])
    levels = pcr.build_overviews(g, 3, mode)
    for b in range(3):
        for lv, want in zip(levels, M.pyramid(arrays[b], 3, mode)):
            assert lv.band_desc(b).name == g.band_desc(b).name
            M.bits_equal(M.grid_bands(lv)[b], want, f"band {b}")


def test_special_values():
    inf, nan, fmax = np.float32(np.inf), np.float32(np.nan), np.finfo(np.float32).max
    a = np.array([[inf, -inf, fmax, fmax, -0.0, -0.0, nan, nan],
                  [1.0, 2.0, fmax, 1.0, -0.0, -0.0, nan, nan]], np.float32)
    g = M.make_grid([a])
    got = M.grid_bands(pcr.build_overviews(g, 1, "average")[0])[0]
    M.bits_equal(got, M.down(a), "special values")
    assert got.view(np.uint32)[0, 0] == 0x7FC00000                       # Inf + -Inf: the one NaN, whatever the machine's
    assert got[0, 1] == inf                                              # overflow is a value
    assert got.view(np.uint32)[0, 2] == 0x80000000                       # four -0.0 stay -0.0
    assert got.view(np.uint32)[0, 3] == 0x7FC00000                       # no valid cell
    odd = np.array([[np.float32(1.0), np.float32(2.0), np.float32(4.0)]], np.float32)      # 3 x 1: one cell right of the source
    M.bits_equal(M.grid_bands(pcr.build_overviews(M.make_grid([odd]), 1, "average")[0])[0],
                 np.array([[1.5, 4.0]], np.float32), "ragged edge")


# ---- the level rule ---------------------------------------------------------------------------------------------------
def test_level_rule():
    def sizes(w, h, levels):
        return [(g.cols(), g.rows()) for g in pcr.build_overviews(pcr.Grid.create(w, h, [pcr.BandDesc()]), levels)]
    assert sizes(1024, 512, -1) == [(512, 256)]
    assert sizes(511, 511, -1) == []
    assert sizes(4096, 4096, -1) == [(2048, 2048), (1024, 1024), (512, 512), (256, 256)]
    assert sizes(3, 5, 0) == []
    assert sizes(3, 5, 3) == [(2, 3), (1, 2), (1, 1)]
    g = pcr.Grid.create(3, 5, [pcr.BandDesc()])
    with pytest.raises(RuntimeError, match="more overview levels"):
        pcr.build_overviews(g, 4)
    with pytest.raises(RuntimeError, match="more overview levels"):
        pcr.build_overviews(pcr.Grid.create(1, 1, [pcr.BandDesc()]), 1)
    with pytest.raises(RuntimeError, match="unknown overview_resampling"):
        pcr.build_overviews(g, 1, "cubic")
    assert pcr.build_overviews(g, 0, "cubic") == []                       # the string is looked at only when levels are asked for


def test_bad_resampling_is_refused_only_with_overviews(tmp_path):
    a = M.values(40, 30, seed=5)
    g, cfg = M.make_grid([a]), grid_config(40, 30)
    opt = pcr.GeoTiffOptions()
    assert opt.overviews == 0
    opt.overview_resampling = "cubic"
    p = str(tmp_path / "a.tif")
    pcr.write_geotiff(p, g, cfg, opt)                                     # as before: never looked at
    assert pcr.read_geotiff_overviews(p) == []
    opt.overviews = 2
    with pytest.raises(RuntimeError, match="unknown overview_resampling"):
        pcr.write_geotiff(p, g, cfg, opt)


# ---- the file -----------------------------------------------------------------------------------------------------------
def walk_ifds(path):
    """[(tags in file order, {tag: first value})] for every directory of a little-endian TIFF / BigTIFF."""
    d = open(path, "rb").read()
    big = struct.unpack_from("<H", d, 2)[0] == 43
    off = struct.unpack_from("<Q", d, 8)[0] if big else struct.unpack_from("<I", d, 4)[0]
    out = []
    while off:
        n = struct.unpack_from("<Q", d, off)[0] if big else struct.unpack_from("<H", d, off)[0]
        p = off + (8 if big else 2)
        order, first = [], {}
        for _ in range(n):
            tag, typ = struct.unpack_from("<HH", d, p)
            cnt = struct.unpack_from("<Q", d, p + 4)[0] if big else struct.unpack_from("<I", d, p + 4)[0]
            val = d[p + (12 if big else 8):p + (20 if big else 12)]
            order.append(tag)
            if cnt == 1 and typ in (3, 4):
                first[tag] = struct.unpack_from("<H" if typ == 3 else "<I", val)[0]
            p += 20 if big else 12
        out.append((order, first))
        off = struct.unpack_from("<Q", d, p)[0] if big else struct.unpack_from("<I", d, p)[0]
        assert len(out) < 64
    return out


@pytest.fixture(scope="module")
def file_case():
    W, H = 301, 203
    arrays = [M.values(W, H, seed=11), M.values(W, H, seed=12, nan_fraction=0.5)]
    return W, H, arrays, {m: [M.pyramid(a, 3, m) for a in arrays] for m in MODES}


@pytest.mark.parametrize("compress", ["NONE", "LZW", "DEFLATE"])
@pytest.mark.parametrize("tiled", [True, False])
@pytest.mark.parametrize("big", [True, False])
def test_file_levels(tmp_path, file_case, compress, tiled, big):
    W, H, arrays, want = file_case
    mode = "average" if tiled else "nearest"
    g, cfg = M.make_grid(arrays, ["mean", "count"]), grid_config(W, H)
    opt = pcr.GeoTiffOptions()
    opt.compress, opt.bigtiff = compress, big
    opt.tile_width, opt.tile_height = (64, 64) if tiled else (0, 0)
    plain = str(tmp_path / "plain.tif")
    pcr.write_geotiff(plain, g, cfg, opt)
    opt.overviews, opt.overview_resampling = 3, mode
    p = str(tmp_path / "ov.tif")
    pcr.write_geotiff(p, g, cfg, opt)

    assert pcr.read_geotiff_overviews(p) == [(151, 102), (76, 51), (38, 26)]
    assert pcr.read_geotiff_overviews(plain) == []
    for b in range(2):
        M.bits_equal(pcr.read_geotiff_band(p, b), arrays[b], "level 0")
        M.bits_equal(pcr.read_geotiff_band(p, b, 0), pcr.read_geotiff_band(plain, b), "level 0 as without overviews")
        for k in range(3):
            M.bits_equal(pcr.read_geotiff_band(p, b, k + 1), want[mode][b][k], f"band {b} level {k + 1}")
    with pytest.raises(RuntimeError, match="out of range"):
        pcr.read_geotiff_band(p, 0, 4)
    # everything read_geotiff_info and read_geotiff_band_names answer is what the plain file answers
    ia, ib = pcr.read_geotiff_info(p), pcr.read_geotiff_info(plain)
    assert ia[:3] == ib[:3] == (W, H, 2) and ia[3].epsg == ib[3].epsg == 32618
    assert (ia[4].min_x, ia[4].min_y, ia[4].max_x, ia[4].max_y) == (ib[4].min_x, ib[4].min_y, ib[4].max_x, ib[4].max_y)
    assert pcr.read_geotiff_band_names(p) == pcr.read_geotiff_band_names(plain) == ["mean", "count"]

    # the directories: IFD 0 as without overviews; the levels flagged, sized, laid out like level 0, without georeferencing
    ifds, ifds_plain = walk_ifds(p), walk_ifds(plain)
    assert len(ifds) == 4 and len(ifds_plain) == 1
    assert ifds[0][0] == ifds_plain[0][0] and 254 not in ifds[0][0]
    for k, (order, first) in enumerate(ifds):
        assert order == sorted(order) and len(set(order)) == len(order)
        if k == 0:
            continue
        assert first[254] == 1
        assert (first[256], first[257]) == [(151, 102), (76, 51), (38, 26)][k - 1]
        for tag in (259, 262, 277, 284):
            assert first[tag] == ifds[0][1][tag], tag
        assert {258, 338, 339, 42113} <= set(order)
        assert not {33550, 33922, 34264, 34735, 34737, 42112} & set(order)
        if tiled:
            assert (first[322], first[323]) == (64, 64) and 273 not in order
        else:
            assert first[278] == max(1, min(first[257], 65536 // first[256])) and 322 not in order


@pytest.mark.parametrize("tiled", [True, False])
@pytest.mark.parametrize("big", [True, False])
@pytest.mark.parametrize("compress", ["NONE", "LZW", "DEFLATE"])
def test_pillow_reads_every_page(tmp_path, compress, big, tiled):
    from PIL import Image
    W, H = 301, 203
    a = M.values(W, H, seed=21)
    opt = pcr.GeoTiffOptions()
    opt.compress, opt.bigtiff, opt.overviews = compress, big, 3
    opt.tile_width, opt.tile_height = (64, 64) if tiled else (0, 0)
    p = str(tmp_path / "one.tif")
    pcr.write_geotiff(p, M.make_grid([a]), grid_config(W, H), opt)
    want = [a] + M.pyramid(a, 3)
    with Image.open(p) as im:
        assert im.n_frames == 4
        for k in range(4):
            im.seek(k)
            assert im.size == (want[k].shape[1], want[k].shape[0]) and im.mode == "F"
            M.bits_equal(np.array(im), want[k], f"page {k}")


def test_supplied_levels(tmp_path):
    W, H = 129, 65
    a = M.values(W, H, seed=31)
    g, cfg = M.make_grid([a]), grid_config(W, H)
    levels = pcr.build_overviews(g, 2, "nearest")
    p = str(tmp_path / "s.tif")
    pcr.write_geotiff(p, g, cfg, pcr.GeoTiffOptions(), overviews=levels)
    assert pcr.read_geotiff_overviews(p) == [(65, 33), (33, 17)]
    M.bits_equal(pcr.read_geotiff_band(p, 0, 2), M.pyramid(a, 2, "nearest")[1], "supplied level 2")
    pcr.write_geotiff(p, g, cfg, pcr.GeoTiffOptions(), overviews=None)
    assert pcr.read_geotiff_overviews(p) == []
    wrong = pcr.build_overviews(M.make_grid([M.values(W + 2, H, seed=32)]), 1)
    with pytest.raises(RuntimeError, match="cascade's size"):
        pcr.write_geotiff(p, g, cfg, pcr.GeoTiffOptions(), overviews=wrong)
    with pytest.raises(RuntimeError, match="cascade's size"):
        pcr.write_geotiff(p, g, cfg, pcr.GeoTiffOptions(), overviews=[levels[1]])
    two_bands = pcr.build_overviews(M.make_grid([a, a]), 1)
    with pytest.raises(RuntimeError, match="band count"):
        pcr.write_geotiff(p, g, cfg, pcr.GeoTiffOptions(), overviews=two_bands)


def test_classic_tiff_size_check_covers_the_levels(tmp_path):
    # (the 4 GB bound itself cannot be reached in a quick test: this pins that a classic file with levels stays readable
    #  and that its directory offsets are 32-bit)
    a = M.values(64, 64, seed=41)
    opt = pcr.GeoTiffOptions()
    opt.bigtiff, opt.overviews, opt.compress = False, 6, "NONE"
    p = str(tmp_path / "c.tif")
    pcr.write_geotiff(p, M.make_grid([a]), grid_config(64, 64), opt)
    assert open(p, "rb").read(4) == b"II\x2a\x00"
    assert [s for s in pcr.read_geotiff_overviews(p)] == [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    M.bits_equal(pcr.read_geotiff_band(p, 0, 6), M.pyramid(a, 6)[5], "1x1 level")


def test_tiled_writer_and_cloud_optimized_refuse(tmp_path):
    cfg = grid_config(128, 128)
    opt = pcr.GeoTiffOptions()
    opt.overviews = -1
    with pytest.raises(RuntimeError):
        pcr.TiledGeoTiffWriter.open(str(tmp_path / "t.tif"), cfg, ["a"], opt)
    opt = pcr.GeoTiffOptions()
    opt.cloud_optimized = True
    with pytest.raises(RuntimeError, match="not implemented.*overviews"):
        pcr.write_geotiff(str(tmp_path / "c.tif"), M.make_grid([M.values(128, 128, seed=1)]), cfg, opt)


# ---- pipelines ------------------------------------------------------------------------------------------------------------
def host_pipeline_cfg(W, H, threads):
    cfg = pcr.PipelineConfig()
    cfg.grid.bounds = pcr.BBox(0.0, 0.0, float(W), float(H))
    cfg.grid.cell_size_x, cfg.grid.cell_size_y = 1.0, -1.0
    cfg.grid.compute_dimensions()
    cfg.exec_mode = pcr.ExecutionMode.CPU
    cfg.cpu_threads = threads
    specs = []
    for t in (pcr.ReductionType.Average, pcr.ReductionType.Count):
        r = pcr.ReductionSpec()
        r.value_channel, r.type = "value", t
        specs.append(r)
    cfg.reductions = specs
    return cfg


def cloud(W, H, n, seed):
    rng = np.random.default_rng(seed)
    c = pcr.PointCloud.create(n)
    c.set_x_array(rng.uniform(0.0, W * 0.8, n))                           # the right fifth stays empty: NaN cells
    c.set_y_array(rng.uniform(0.0, H, n))
    c.add_channel("value", pcr.DataType.Float32)
    c.set_channel_array_f32("value", rng.normal(0.0, 100.0, n).astype(np.float32))
    return c


@pytest.mark.parametrize("threads", [1, 3])
def test_host_pipeline_write_cog(tmp_path, threads):
    W, H = 600, 520
    pts = cloud(W, H, 150_000, seed=51)
    for cog in (True, False):
        cfg = host_pipeline_cfg(W, H, threads)
        cfg.output_path, cfg.write_cog = str(tmp_path / f"p{int(cog)}.tif"), cog
        pipe = pcr.Pipeline.create(cfg)
        assert pipe is not None, pcr.pipeline_create_error()
        pipe.ingest(pts)
        pipe.finalize()
        bands = M.grid_bands(pipe.result())
        assert np.isnan(bands[0]).any() and not np.isnan(bands[0]).all()
        assert pcr.read_geotiff_overviews(cfg.output_path) == ([(300, 260)] if cog else [])       # 520 / 2 >= 256 > 520 / 4
        for b in range(2):
            M.bits_equal(pcr.read_geotiff_band(cfg.output_path, b), bands[b], "level 0")
            if cog:
                M.bits_equal(pcr.read_geotiff_band(cfg.output_path, b, 1), M.down(bands[b]), f"band {b} level 1")


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------
def test_downsample2_argument_errors_need_no_gpu():
    A = load_cabi()
    L = A.lib()
    src = C.c_void_p(0x1000)                       # never dereferenced: every call below is refused before any HIP call
    dst = (C.c_void_p * 8)(*[0x2000 + 0x100 * k for k in range(8)])
    def call(s=src, w=16, h=16, stride=16, d=dst, levels=2, mode=0):
        return L.pcr_hip_downsample2(s, w, h, stride, d, levels, mode, None)
    for kw, msg in ((dict(s=None), b"null argument"), (dict(d=None), b"null argument"),
                    (dict(w=0), b"must be positive"), (dict(h=-1), b"must be positive"), (dict(levels=0), b"levels must be positive"),
                    (dict(stride=15), b"src_stride smaller than width"), (dict(mode=2), b"unknown mode"),
                    (dict(levels=5), b"more levels than halvings"), (dict(w=1, h=1, stride=1, levels=1), b"more levels than halvings")):
        assert call(**kw) == 1, kw
        assert msg in L.pcr_hip_last_error(), (kw, L.pcr_hip_last_error())
    holes = (C.c_void_p * 8)(0x2000, None)
    assert call(d=holes) == 1 and b"null level pointer" in L.pcr_hip_last_error()
    assert L.pcr_hip_abi_version() == 5
