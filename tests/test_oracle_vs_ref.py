"""Pins the CPU oracle against the reference's OWN code.

 * test_*_fixture: against tests/golden/ref_vectors.npz (outputs of oracle/_ref, committed);
   runs everywhere, including the GPU box where /root/reference does not exist.
 * test_*_live: against oracle/_ref/libpcr_ref.so when it was built (development container), and against
   its outputs recorded in tests/golden/ref_live.npz (make_ref_live.py) everywhere else.

Both sides fold points sequentially in input order with the same fp32 operations, so the
comparison is BIT-EXACT on the raw tile state and on the finalized tile.
"""
import os
import sys

import numpy as np
import pytest

import pcr_oracle_py as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import cases                      # noqa: E402
import make_ref_vectors as MRV    # noqa: E402
import make_ref_live as MRL       # noqa: E402

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vectors.npz")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    assert np.array_equal(nan_a, nan_b), what + ": NaN mask"
    assert np.array_equal(_bits(a[~nan_a]), _bits(b[~nan_b])), what + ": bits differ"


@pytest.fixture(scope="module")
def fixture_vectors():
    return np.load(FIX)


@pytest.fixture(scope="module")
def live_vectors():
    return np.load(MRL.PATH)


@pytest.mark.parametrize("case", cases.GLYPH_CASES, ids=lambda c: c["name"])
def test_glyph_fixture(case, fixture_vectors):
    L = O.lib()
    st, fin = MRV.run_glyph(L.pcro_accumulate_glyph, L.pcro_init_state, L.pcro_finalize_state, case)
    _same(st, fixture_vectors[case["name"] + "/state"], case["name"] + " state")
    _same(fin, fixture_vectors[case["name"] + "/final"], case["name"] + " final")
    assert np.isfinite(st).all() and (st != 0).any()


@pytest.mark.parametrize("case", cases.POINT_CASES, ids=lambda c: c["name"])
def test_point_fixture(case, fixture_vectors):
    L = O.lib()
    st, fin = MRV.run_point(L.pcro_accumulate, L.pcro_init_state, L.pcro_finalize_state, case)
    _same(st, fixture_vectors[case["name"] + "/state"], case["name"] + " state")
    _same(fin, fixture_vectors[case["name"] + "/final"], case["name"] + " final")
    if case["rtype"] == cases.SUM:      # quirk Q2: empty cell finalizes to 0.0 for Sum, NaN otherwise
        assert (fin == 0.0).any() and not np.isnan(fin).any()
    else:
        assert np.isnan(fin).any(), "case should contain empty cells"


def test_live_ref_matches_fixture_and_oracle():
    R, L = O.ref_lib(), O.lib()
    fx = np.load(FIX)
    for case in cases.GLYPH_CASES:
        st_o, fin_o = MRV.run_glyph(L.pcro_accumulate_glyph, L.pcro_init_state,
                                    L.pcro_finalize_state, case)
        if R is None:
            st_r, fin_r = fx[case["name"] + "/state"], fx[case["name"] + "/final"]
        else:
            st_r, fin_r = MRV.run_glyph(R.pcr_ref_accumulate_glyph, R.pcr_ref_init_state,
                                        R.pcr_ref_finalize_state, case)
        _same(st_o, st_r, case["name"])
        _same(fin_o, fin_r, case["name"])
        _same(st_r, fx[case["name"] + "/state"], case["name"] + " (fixture stale?)")
    for case in cases.POINT_CASES:
        st_o, fin_o = MRV.run_point(L.pcro_accumulate, L.pcro_init_state, L.pcro_finalize_state, case)
        if R is None:
            st_r, fin_r = fx[case["name"] + "/state"], fx[case["name"] + "/final"]
        else:
            st_r, fin_r = MRV.run_point(R.pcr_ref_accumulate, R.pcr_ref_init_state, R.pcr_ref_finalize_state, case)
        _same(st_o, st_r, case["name"])
        _same(fin_o, fin_r, case["name"])


def test_live_ref_merge_state(live_vectors):
    R, L = O.ref_lib(), O.lib()
    for rt, a, b in MRL.merge_inputs(L):
        a2 = a.copy()
        if R is None:
            a = live_vectors[f"merge/{rt}"]
        else:
            assert R.pcr_ref_merge_state(rt, a.ctypes.data, b.ctypes.data, 64) == 0
            _same(a, live_vectors[f"merge/{rt}"], f"merge {rt} (fixture stale?)")
        assert L.pcro_merge_state(rt, a2.ctypes.data, b.ctypes.data, 64) == 0
        _same(a, a2, f"merge {rt}")


def test_live_ref_glyph_quirk_probes(known_answers, live_vectors):
    """The survey-verified glyph probes, re-checked against the reference code itself (without oracle/_ref: against what it
    returned, recorded, which the oracle must reproduce bit for bit)."""
    R, L = O.ref_lib(), O.lib()
    for i, c in enumerate(known_answers["glyph"]):
        if R is None:
            band = MRL.probe_band(L.pcro_accumulate_glyph, c)
            if band is None:
                continue   # tile clipping needs the router; covered at state level by *_clip cases
            _same(band, live_vectors[f"probe/{i}"], f"probe case {i}: oracle vs recorded reference")
        else:
            band = MRL.probe_band(R.pcr_ref_accumulate_glyph, c)
            if band is None:
                continue
            _same(band, live_vectors[f"probe/{i}"], f"probe case {i} (fixture stale?)")
        for row, col, val in c.get("probes", []):
            assert band[row, col] == pytest.approx(val, rel=c["rtol"])
        if "cells_set" in c:
            assert sorted([int(r), int(cc)] for r, cc in np.argwhere(band != 0)) == sorted(c["cells_set"])


@pytest.mark.parametrize("rname", MRL.LATTICE_RTYPES)
@pytest.mark.parametrize("glyph", MRL.LATTICE_GLYPHS)
def test_live_ref_glyphs_on_cell_edges(glyph, rname, live_vectors):
    """Footprints whose centre is on a cell edge or an ulp off it (tests/routing_lattice.py): the reference places them by
    floor((wx - min_x) * (1 / cell_size)), a product, which on such points is not always the cell a division gives.  The
    restatement against the reference's own code, bit for bit on the raw state (without oracle/_ref: against the digest of what
    it returned)."""
    R, L = O.ref_lib(), O.lib()
    grid = MRL.RL.grid("ref_tile")
    dx, dy = MRL.RL.disagreements(grid, *MRL.RL.cloud("ref_tile")[:2])
    assert dx.sum() >= 50 and dy.sum() >= 50, "the cloud no longer holds points the two formulas place differently"
    rt = MRL.LATTICE_RTYPES[rname]
    recorded = str(live_vectors[f"lattice/{glyph}/{rname}"])
    st_o = MRL.lattice_state(L.pcro_accumulate_glyph, glyph, rt)
    if R is not None:
        st_r = MRL.lattice_state(R.pcr_ref_accumulate_glyph, glyph, rt)
        assert cases.digest(st_r) == recorded, f"{glyph}/{rname} (fixture stale?)"
        _same(st_o, st_r, f"{glyph}/{rname} state")
    assert cases.digest(st_o) == recorded, f"{glyph}/{rname} vs recorded reference"
    assert np.isfinite(st_o).all() and (st_o != 0).any()


@pytest.mark.parametrize("block", range(8))
def test_live_ref_matches_oracle_on_random_glyph_cases(block, live_vectors):
    """320 random accumulate_glyph() calls, the C restatement against the reference's own code (without oracle/_ref: against
    the digests of what it returned, tests/golden/ref_live.npz): raw tile state and finalized tile bit for bit (both fold the
    points in input order with the same fp32 operations) for the 206 the reference accepts; the 114 it refuses (Max / Min
    through a glyph) the restatement refuses too."""
    R, L = O.ref_lib(), O.lib()
    for seed in range(block * 40, block * 40 + 40):
        case = cases.random_glyph_case(seed)
        recorded = tuple(str(s) for s in live_vectors[f"random/{seed}"])
        if R is not None:
            assert MRL.random_case_record(R, case) == recorded, f"{case['name']} (fixture stale?)"
        if recorded == ("refused",):
            # the reference refuses the combination (e.g. a reduction its glyph path does not take): the oracle must too
            with pytest.raises(AssertionError):
                MRV.run_glyph(L.pcro_accumulate_glyph, L.pcro_init_state, L.pcro_finalize_state, case)
            continue
        st_o, fin_o = MRV.run_glyph(L.pcro_accumulate_glyph, L.pcro_init_state, L.pcro_finalize_state, case)
        if R is not None:
            st_r, fin_r = MRV.run_glyph(R.pcr_ref_accumulate_glyph, R.pcr_ref_init_state, R.pcr_ref_finalize_state, case)
            _same(st_o, st_r, f"{case['name']} state ({case})")
            _same(fin_o, fin_r, f"{case['name']} final ({case})")
        assert (cases.digest(st_o), cases.digest(fin_o)) == recorded, f"{case['name']} vs recorded reference ({case})"
