"""CPU: Pipeline.ingest on the host engine (ExecutionMode.CPU) reprojects a cloud whose CRS differs from the grid's
(PipelineConfig.auto_reproject), and nothing else changes."""
import numpy as np
import pytest

import reproject_common as R

pcr = pytest.importorskip("pcr")
O = pytest.importorskip("pcr_oracle_py")

SIZE, N = 96, 60_000


@pytest.fixture(scope="module")
def case():
    x, y, v = R.cell_points(SIZE, N)
    lon, lat = R.utm_inverse_np(x, y, 18)
    return x, y, v, lon, lat, R.oracle_bands(O, SIZE, x, y, v)


def run(cfg, clouds):
    p = pcr.Pipeline.create(cfg)
    assert p is not None, pcr.pipeline_create_error()
    assert p.engine() == "host"
    for c in clouds:
        p.ingest(c)
    p.finalize()
    return p.result()


def cpu_cfg(**kw):
    return R.make_config(pcr, SIZE, pcr.ExecutionMode.CPU, **kw)


def test_lonlat_cloud_lands_in_the_utm_cells(case):
    x, y, v, lon, lat, want = case
    cloud = R.make_cloud(pcr, lon, lat, v, pcr.CRS.from_epsg(4326))
    R.check_bands(run(cpu_cfg(), [cloud]), want, "4326 -> 32618")


def test_target_crs_when_the_grid_has_none(case):
    x, y, v, lon, lat, want = case
    cfg = cpu_cfg(grid_crs=pcr.CRS())
    cfg.target_crs = pcr.CRS.from_epsg(32618)
    R.check_bands(run(cfg, [R.make_cloud(pcr, lon, lat, v, pcr.CRS.from_epsg(4326))]), want, "target_crs")


def test_wkt_tagged_cloud_and_grid(case):
    x, y, v, lon, lat, want = case
    cloud = R.make_cloud(pcr, lon, lat, v, pcr.CRS.from_wkt(R.WKT_4326))
    R.check_bands(run(cpu_cfg(grid_crs=pcr.CRS.from_wkt(R.WKT1_UTM)), [cloud]), want, "WKT")


def test_auto_reproject_off_keeps_todays_result(case):
    x, y, v, lon, lat, want = case
    cfg = cpu_cfg()
    cfg.auto_reproject = False
    g = run(cfg, [R.make_cloud(pcr, lon, lat, v, pcr.CRS.from_epsg(4326))])
    for i in range(3):
        assert np.isnan(np.asarray(g.band_array(i))).all()        # lon/lat are far outside the UTM bounds


def test_unidentified_or_equal_crs_is_not_transformed(case):
    x, y, v, lon, lat, want = case
    # a cloud already in UTM metres, tagged with a WKT that names no top-level authority: ingested as it is
    g = run(cpu_cfg(), [R.make_cloud(pcr, x, y, v, pcr.CRS.from_wkt('PROJCS["fixture"]'))])
    R.check_bands(g, want, "unidentified")
    g = run(cpu_cfg(), [R.make_cloud(pcr, x, y, v, pcr.CRS.from_epsg(32618))])
    R.check_bands(g, want, "same code")
    g = run(cpu_cfg(), [R.make_cloud(pcr, x, y, v, None)])
    R.check_bands(g, want, "untagged")


def test_callers_cloud_is_not_modified(case):
    x, y, v, lon, lat, want = case
    cloud = R.make_cloud(pcr, lon, lat, v, pcr.CRS.from_epsg(4326))
    run(cpu_cfg(), [cloud])
    assert np.array_equal(cloud.x_array(), lon) and np.array_equal(cloud.y_array(), lat)
    assert cloud.crs().epsg == 4326


def test_unsupported_pair_is_refused_and_accumulates_nothing(case):
    x, y, v, lon, lat, want = case
    half = N // 2
    good = R.make_cloud(pcr, lon[:half], lat[:half], v[:half], pcr.CRS.from_epsg(4326))
    bad = R.make_cloud(pcr, lon[half:], lat[half:], v[half:], pcr.CRS.from_epsg(2263))
    p = pcr.Pipeline.create(cpu_cfg())
    p.ingest(good)
    with pytest.raises(RuntimeError) as e:
        p.ingest(bad)
    assert "2263" in str(e.value) and "32618" in str(e.value)
    p.finalize()
    R.check_bands(p.result(), R.oracle_bands(O, SIZE, x[:half], y[:half], v[:half]), "after refusal")


def test_ingest_file_takes_the_crs_of_the_file(case, tmp_path):
    x, y, v, lon, lat, want = case
    path = str(tmp_path / "lonlat.pcrp")
    pcr.write_point_cloud(path, R.make_cloud(pcr, lon, lat, v, pcr.CRS.from_wkt(R.WKT_4326)))
    p = pcr.Pipeline.create(cpu_cfg())
    assert p.ingest_file(path, chunk_points=7_000) == N
    p.finalize()
    R.check_bands(p.result(), want, "ingest_file")
