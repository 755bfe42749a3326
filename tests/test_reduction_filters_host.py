"""ReductionSpec.filter on the host engine, and everything about it that needs no GPU: the NumPy model of
reduction_filters_common against ExecutionMode.CPU, the refusals at create and at ingest, the C-ABI's argument errors."""
import ctypes as C

import numpy as np
import pytest

import pcr
import reduction_filters_common as RF
from conftest import load_cabi


def test_the_spec_filter_is_changed_in_place_from_python():
    spec = pcr.ReductionSpec()
    assert spec.filter.empty()
    spec.filter.add("classification", pcr.CompareOp.Equal, 2.0)
    spec.filter.add_in_set("return_number", [1.0, 2.0])
    assert [p.channel_name for p in spec.filter.predicates] == ["classification", "return_number"]
    assert spec.filter.predicates[0].value == 2.0 and list(spec.filter.predicates[1].value_set) == [1.0, 2.0]


def test_the_model_routes_like_the_oracle():
    import pcr_oracle_py as O
    c = RF.make_points(1027, 3)
    og = O.make_grid((0.0, 0.0, 40.0, 24.0), tile=(16, 16))
    cell = RF.cells_of(RF.GRID, c["x"], c["y"])
    for i in range(0, 1027, 3):
        col, row, ok = O.world_to_cell(og, float(c["x"][i]), float(c["y"][i]))
        assert cell[i] == (row * og.width + col if ok else -1)


@pytest.mark.parametrize("n", RF.SIZES)
def test_mixed_pipeline(n):
    RF.check_mixed("cpu", n)


@pytest.mark.parametrize("n", RF.SIZES)
def test_all_specs_filtered_flags_come_from_every_point(n):
    RF.check_all_filtered("cpu", n)


@pytest.mark.parametrize("n", RF.SIZES)
def test_with_a_pipeline_filter_as_well(n):
    RF.check_with_cfg_filter("cpu", n)


@pytest.mark.parametrize("name", list(RF.CFG_ONLY_PREDS))
@pytest.mark.parametrize("n", RF.CFG_ONLY_SIZES)
def test_a_pipeline_filter_alone(n, name):
    RF.check_cfg_filter_only("cpu", n, RF.CFG_ONLY_PREDS[name])


def test_no_case_of_a_pipeline_filter_alone_passes_vacuously():
    for n in RF.CFG_ONLY_SIZES:
        c = RF.cfg_only_points(n)
        inside = RF.cells_of(RF.GRID, c["x"], c["y"]) >= 0
        for name, preds in RF.CFG_ONLY_PREDS.items():
            keep = RF.conj_mask(c, preds)
            if name == "none":
                assert not keep.any()
            elif n >= 63:
                assert (keep & inside).any() and not keep.all(), f"{name}, {n} points"
    c = RF.cfg_only_points(259)
    assert (RF.conj_mask(c, RF.SEVENTEEN) & (RF.cells_of(RF.GRID, c["x"], c["y"]) >= 0)).any()
    assert len({p[:2] + (str(p[2]),) for p in RF.CFG_ONLY_PREDS["sixteen"]}) == 16 and len(RF.SEVENTEEN) == 17
    assert {p[0] for p in RF.CFG_ONLY_PREDS["five channels"]} == set(RF.CHANNELS)
    assert np.isnan(RF.cfg_only_points(63)["q"]).any()


def test_a_pipeline_filter_of_17_predicates():
    RF.check_cfg_filter_too_long("cpu")


def test_predicate_edge_cases():
    RF.check_predicate_edges("cpu")


def test_against_pipelines_of_their_own():
    RF.check_against_own_pipelines("cpu")


def test_the_bits_do_not_depend_on_the_thread_count():
    c = RF.make_points(20000, 11)
    out = []
    for threads in (1, 3, 8):
        p = RF.create("cpu", RF.MIXED, [("ret", "LessEqual", 2.0)], cpu_threads=threads)
        p.ingest(RF.make_cloud(c, "cpu"))
        p.finalize()
        out.append(RF.bands(p))
    for other in out[1:]:
        for b, (u, w) in enumerate(zip(out[0], other)):
            RF.assert_bits(u, w, f"band {b}")


def test_refusals():
    RF.check_refusals("cpu")


def test_two_ingests_and_a_checkpoint(tmp_path):
    RF.check_two_ingests_and_checkpoint("cpu", tmp_path)


def test_a_las_file_with_a_spec_filter_on_classification(tmp_path):
    RF.check_las("cpu", tmp_path)


def test_filtered_line_groups():
    RF.check_line("cpu")


def test_filter_classes_argument_errors_need_no_gpu():
    A = load_cabi()
    L = A.lib()
    preds = (A.Predicate * 2)()
    for k in range(2):
        preds[k].d_channel, preds[k].op, preds[k].value = 4096, 0, 1.0      # (never dereferenced: every call below is refused first)
    words = (C.c_uint32 * 9)(*([1] * 9))
    call = lambda p, n_pred, w, n_cls: L.pcr_hip_filter_classes(p, n_pred, w, n_cls, 64, 4096, 64, None, None)
    assert call(preds, 2, None, 1) == 1 and b"null class table" in L.pcr_hip_last_error()
    assert call(None, 2, words, 1) == 1 and b"null predicate table" in L.pcr_hip_last_error()
    assert call(preds, 2, words, 0) == 1 and b"1..8 classes" in L.pcr_hip_last_error()
    assert call(preds, 2, words, 9) == 1 and b"1..8 classes" in L.pcr_hip_last_error()
    words[1] = 4                                                            # bit 2 of a table of two
    assert call(preds, 2, words, 2) == 1 and b"outside the table" in L.pcr_hip_last_error()
    assert L.pcr_hip_engine_touch(None, None, None, 8) == 1 and b"null engine" in L.pcr_hip_last_error()
    assert L.pcr_hip_abi_version() == 5
