"""Individual trees on the MI355X: pcr_hip_trees, _count and _table through the C-ABI (rows on 16 bytes and not, windows of
strided planes between sentinels, the tile's edges, long chains, degenerate bands), behind pcr.segment_trees on Device grids,
and the HIP engine's PipelineConfig.trees.  Everything BIT FOR BIT against the host twin, which tests/test_trees.py holds to
the brute-force model of the contract."""
import ctypes as C

import numpy as np
import pytest

import ground_filter_common as G
import overviews_common as M
import pcr
import trees_common as T
from conftest import load_cabi

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = float("inf")
GPU, CPU = pcr.ExecutionMode.GPU, pcr.ExecutionMode.CPU
LOCATIONS = [pcr.MemoryLocation.Host, pcr.MemoryLocation.Device]
# (rows, cols).  The first kernel's tile is 64 columns x 32 rows: one below, on and one above it both ways
SHAPES = [(1, 1), (1, 7), (7, 1), (31, 63), (32, 64), (33, 65), (31, 65), (33, 63), (70, 130)]

FIELDS = {}


def field(h, w, seed=1):
    if (h, w, seed) not in FIELDS:
        FIELDS[(h, w, seed)] = T.canopy(w, h, seed)
    return FIELDS[(h, w, seed)]


def check_device(a, what, **kw):
    """The kernels on `a` against the host twin; -> (the result, the jumping rounds that changed a pointer)."""
    A = load_cabi()
    dev_kw = {k: kw.pop(k) for k in ("stride", "offset") if k in kw}
    want = T.host_cabi(A, a, **kw)
    got, rounds = T.device_cabi(A, a, **dev_kw, **kw)
    T.same_result(got, want, what)
    return got, rounds


@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_the_host_twin(shape):
    a = field(*shape)
    h, w = shape
    if shape == (70, 130):
        T.exercises_the_rules(a, T.model(a))
    for offset in (0, 3):
        for stride in (w, w + 5):
            check_device(a, f"{shape} offset {offset} stride {stride}", offset=offset, stride=stride)


@pytest.mark.parametrize("kw", [dict(max_radius_cells=1), dict(max_radius_cells=32, window_base=20.0, window_slope=1.5),
                                dict(max_radius_cells=32, window_base=70.0, window_slope=0.0),
                                dict(window_base=0.0, window_slope=0.0), dict(window_base=2.5, window_slope=0.0),
                                dict(min_height=5.0, min_crown_height=1.0, crown_ratio=0.8, max_crown_radius=3.0),
                                dict(crown_ratio=0.0, max_crown_radius=INF, min_crown_height=-5.0)])
def test_parameters(kw):
    a = field(70, 130, 2)
    got, _ = check_device(a, str(kw), **kw)
    assert len(got["table"]["row"]) >= 1
    check_device(a, str(kw) + " half-metre cells", cell_size_x=0.5, cell_size_y=-0.5, **kw)


def test_height_band_may_be_left_out():
    check_device(field(33, 65), "no height band", want_height=False, stride=70)


@pytest.mark.parametrize("transpose", [False, True])
def test_long_chains_need_many_rounds(transpose):
    z = (5.0 + 0.01 * np.arange(3000)).astype(F32)[None, :]
    z = np.ascontiguousarray(z.T) if transpose else z
    got, rounds = check_device(z, "ramp", crown_ratio=0.0, max_crown_radius=INF)
    assert got["table"]["crown_cells"].tolist() == [3000] and (got["id"] == 1).all()
    # ceil(log2(3000)) + 1 = 13 rounds are enqueued: pure doubling needs 12 of them; jumping in place may read a pointer another
    # lane has just moved and get there sooner
    assert 1 <= rounds <= 13


def test_degenerate_bands():
    nan = np.full((40, 70), np.nan, F32)
    got, rounds = check_device(nan, "all NaN")
    assert len(got["table"]["row"]) == 0 and np.isnan(got["id"]).all() and rounds == 0
    flat = np.full((40, 70), 7.0, F32)                     # R = 1: a cell is a top when no edge neighbour beats it
    got, _ = check_device(flat, "constant")
    assert got["table"]["row"].tolist() == [0] and got["table"]["col"].tolist() == [0]
    rr, cc = np.mgrid[0:40, 0:70]
    assert got["table"]["crown_cells"].tolist() == [int((rr * rr + cc * cc <= 100).sum())]       # max_crown_radius = 10 cells
    got, _ = check_device(flat, "constant, no window", window_base=0.0, window_slope=0.0)        # R = 0: every cell is a top
    assert got["id"].ravel().tolist() == list(range(1, flat.size + 1))
    got, _ = check_device(flat, "constant, wide window", window_base=21.0, window_slope=0.0)    # R = 10
    assert got["table"]["row"].tolist() == [0] and got["table"]["col"].tolist() == [0]
    check_device(M.values(130, 70, 32), "values of every kind", min_height=-1e30, min_crown_height=-1e30)


def test_segment_trees_on_a_device_grid():
    a, b = field(70, 130), field(70, 130, 3)
    g = T.make_grid([a, b])
    sp = T.spec(min_height=3.0, window_slope=0.1)
    for band in (0, 1):
        host, table_h = pcr.segment_trees(g, band, sp, 0.5, -0.5)
        dev, table_d = pcr.segment_trees(g.to(pcr.MemoryLocation.Device), band, sp, 0.5, -0.5)
        assert dev.location() == pcr.MemoryLocation.Device
        assert [dev.band_desc(k).name for k in range(2)] == ["tree_id", "tree_height"]
        x, y = T.grid_bands(dev.to_host()), T.grid_bands(host)
        T.same_result(dict(id=x[0], height=x[1], table=table_d), dict(id=y[0], height=y[1], table=table_h), f"band {band}")
        assert len(table_d["row"]) > 0
    with pytest.raises(RuntimeError, match="max_radius_cells must be between 1 and 32"):
        pcr.segment_trees(g.to(pcr.MemoryLocation.Device), 0, T.spec(max_radius_cells=40))


# ---- the HIP engine's PipelineConfig.trees ---------------------------------------------------------------------------------------
WP, HP = 130, 70
NEW = ["value_1_tree_id", "value_1_tree_height", "low ids", "low tops"]


def pipeline_cfg(mode, location=pcr.MemoryLocation.Host, trees=True, radius=2):
    cfg = G.pipeline_cfg(WP, HP, mode, ground=False, radius=radius)
    cfg.result_location = location
    if trees:
        cfg.trees = [T.band_cfg("value_1"), T.band_cfg("value_2", "low ids", "low tops", min_height=4.0, window_slope=0.2)]
    return cfg


def create(cfg, engine="hip"):
    pipe = pcr.Pipeline.create(cfg)
    assert pipe is not None, pcr.pipeline_create_error()
    assert pipe.engine() == engine
    return pipe


def result_bands(pipe):
    res = pipe.result()
    return G.grid_bands(res if res.location() == pcr.MemoryLocation.Host else res.to_host())


def names_of(pipe):
    res = pipe.result()
    return [res.band_desc(b).name for b in range(res.num_bands())]


@pytest.fixture(scope="module")
def pipe_case():
    (c1, _), (c2, _) = T.canopy_cloud(WP, HP, 1), T.canopy_cloud(WP, HP, 2)
    host = create(pipeline_cfg(CPU), "host")
    want = []
    for c in (c1, c2):
        host.ingest(c)
        host.finalize()
        want.append((G.grid_bands(host.result()), [host.trees(0), host.trees(1)]))
    assert names_of(host) == list(G.BANDS) + NEW
    assert len(want[0][1][0]["row"]) >= 100 and not np.array_equal(want[0][1][0]["row"], want[1][1][0]["row"])
    return c1, c2, want


@pytest.mark.parametrize("wait", [True, False])
@pytest.mark.parametrize("location", LOCATIONS)
def test_pipeline_equals_the_host_engine(pipe_case, location, wait):
    c1, c2, want = pipe_case
    pipe = create(pipeline_cfg(GPU, location))
    A = load_cabi()
    with pytest.raises(RuntimeError, match="no trees entry 0"):
        pipe.trees(0)
    for k, c in enumerate((c1, c2)):                              # finalize twice with an ingest between: the table follows
        pipe.ingest(c)
        if wait:
            pipe.finalize()
        else:
            pipe.finalize_async()                                 # (trees() waits for the stream itself)
        tables = [pipe.trees(0), pipe.trees(1)]
        pipe.synchronize()
        assert names_of(pipe) == list(G.BANDS) + NEW
        got = result_bands(pipe)
        for b in range(7):                                        # Min, Max, Count are exact on both engines: so is what follows
            M.bits_equal(got[b], want[k][0][b], f"finalize {k + 1}, band {b}")
        for e in range(2):
            T.same_result(dict(id=got[3 + 2 * e], height=got[4 + 2 * e], table=tables[e]),
                          dict(id=want[k][0][3 + 2 * e], height=want[k][0][4 + 2 * e], table=want[k][1][e]), f"finalize {k + 1}, entry {e}")
        for b in range(3, 7):                                     # result_band_device() answers for the new bands
            back = np.empty((HP, WP), F32)
            A.check(A.lib().pcr_hip_memcpy_d2h(back.ctypes.data, C.c_void_p(pipe.result_band_device_ptr(b)), back.nbytes, None))
            A.check(A.lib().pcr_hip_stream_synchronize(None))
            M.bits_equal(back, got[b], f"finalize {k + 1}, result_band_device {b}")
        assert pipe.result_band_device_ptr(7) == 0
    with pytest.raises(RuntimeError, match="no trees entry 2"):
        pipe.trees(2)


@pytest.mark.parametrize("location", LOCATIONS)
def test_an_empty_list_changes_nothing(pipe_case, location):
    c1, _, want = pipe_case
    pipe = create(pipeline_cfg(GPU, location, trees=False))
    pipe.ingest(c1)
    pipe.finalize()
    assert names_of(pipe) == list(G.BANDS)
    for b, band in enumerate(result_bands(pipe)):
        M.bits_equal(band, want[0][0][b], f"band {b}")


@pytest.mark.parametrize("location", LOCATIONS)
def test_geotiff_holds_the_new_bands(tmp_path, pipe_case, location):
    c1, _, want = pipe_case
    cfg = pipeline_cfg(GPU, location)
    cfg.output_path = str(tmp_path / "trees.tif")
    pipe = create(cfg)
    pipe.ingest(c1)
    pipe.finalize()
    assert pcr.read_geotiff_band_names(cfg.output_path) == list(G.BANDS) + NEW
    for b in range(7):
        M.bits_equal(pcr.read_geotiff_band(cfg.output_path, b), want[0][0][b], f"file band {b}")
