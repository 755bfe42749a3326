"""The operation-sequence fuzz (tests/sequence_fuzz_common.py) on the HOST engine (ExecutionMode.CPU), and what it rests on.

The existing suites hold the host engine to the oracle, so where the model and the host engine disagree the model is wrong: this
run pins the model on a machine without a GPU, before tests/test_gpu_sequence_fuzz.py holds the HIP engine to it.  The host
engine hands out no plane or flag pointers and has one flavour; the runner drops those ops, the generator draws them all the same
-- test_the_default_seeds_cover_the_situations looks at what was drawn."""
import json
import os

import numpy as np
import pytest

import pcr
import pcr_oracle_py as O
import sequence_fuzz_common as S
import terrain_common as T
from conftest import GOLDEN


@pytest.mark.parametrize("seed", S.DEFAULT_SEEDS)
def test_sequence_on_the_host_engine_equals_the_model(seed, tmp_path):
    S.check_sequence(seed, pcr.ExecutionMode.CPU, "host", tmp_path)


def test_the_default_seeds_cover_the_situations():
    """Every situation the fuzz is for occurs in at least three default seeds; so do the marks the GPU run asserts on."""
    assert len(S.DEFAULT_SEEDS) == 52 and S.DEFAULT_SEEDS[:40] == S.FIRST_SEEDS
    seen = {name: [] for name in S.SITUATIONS}
    marked, wide, mult4 = [], [], []
    for seed in S.DEFAULT_SEEDS:
        case = S.build(seed)
        first = seed in S.FIRST_SEEDS                             # (the marks below are counted over the 40 first seeds, as they were)
        assert 4 <= len(case["ops"]) <= 12 and case["ops"][-1]["op"] == "finalize", seed
        assert 1 <= len(case["specs"]) <= 10, seed
        found = S.situations(case)
        assert found <= set(S.SITUATIONS)
        for name in found:
            seen[name].append(seed)
        marked += [seed] if first and case["marked"] else []
        wide += [seed] if first and case["wide"] else []
        mult4 += [seed] if first and case["grid"]["W"] % 4 == 0 else []
    for name in S.SITUATIONS:
        assert len(seen[name]) >= 3, f"'{name}' occurs in seeds {seen[name]} only"
    assert len(marked) >= 8, f"only seeds {marked} are certain to store bands with their first ingest"
    assert len(wide) >= 2, f"only seeds {wide} have a group of more than {S.MAX_FINALIZE_OUTPUTS} outputs"
    assert 12 <= len(mult4) <= 28, f"W % 4 == 0 in {len(mult4)} of 40 seeds"


def test_the_first_40_seeds_are_the_cases_they_were():
    """Terrain is drawn last and from generators of its own: without every plan's terrain list a seed is, digest for digest,
    the case it was before the fuzz drew terrain (tests/golden/sequence_fuzz_cases.json, make_sequence_fuzz_cases.py)."""
    with open(os.path.join(GOLDEN, "sequence_fuzz_cases.json")) as f:
        want = json.load(f)["sha256"]
    assert sorted(int(s) for s in want) == sorted(S.FIRST_SEEDS)
    for seed in S.FIRST_SEEDS:
        case = S.build(seed)
        for plan in [case["plan"]] + [o["plan"] for o in case["ops"] if o["op"] == "checkpoint" and o["plan"] is not None]:
            del plan["terrain"]
        assert S.case_digest(case) == want[str(seed)], f"seed {seed} is another case than it was"


def test_the_terrain_draw():
    """What the draw promises: 0 to 6 entries, about four plans of ten without; sources that leave under the plan; names
    that do not clash; parameters from the lists; every product and every kind of source drawn."""
    plans = []
    for seed in S.DEFAULT_SEEDS:
        case = S.build(seed)
        for plan in [case["plan"]] + [o["plan"] for o in case["ops"] if o["op"] == "checkpoint" and o["plan"] is not None]:
            plans.append(plan)
            sources = [S.band_name(i, s) for i, s in enumerate(case["specs"])]
            sources += (["dtm"] if plan["ground"] else []) + (["hag"] if plan["ground"] and plan["ground"]["top"] is not None else [])
            names = sources + [S.terrain_band_name(t) for t in plan["terrain"]]
            assert len(plan["terrain"]) <= 6 and len(set(names)) == len(names), seed
            for t in plan["terrain"]:
                assert t["source"] in sources and t["product"] in S.TERRAIN_PRODUCTS and t["z_factor"] in S.TERRAIN_Z, seed
                assert (t["azimuth"], t["altitude"]) in S.TERRAIN_LIGHTS and t["edges"] in (False, True), seed
    empty = sum(not plan["terrain"] for plan in plans)
    assert 0.25 * len(plans) <= empty <= 0.55 * len(plans), f"{empty} of {len(plans)} plans draw no terrain"
    entries = [t for plan in plans for t in plan["terrain"]]
    assert {t["product"] for t in entries} == set(S.TERRAIN_PRODUCTS)
    assert {t["source"].split("_")[1] if t["source"][0] == "r" else t["source"] for t in entries} == set(S.TYPES) | {"dtm", "hag"}
    assert max(len(plan["terrain"]) for plan in plans) == 6
    assert [p.name for p in T.PRODUCTS] == ["SlopeDegrees", "SlopePercent", "Aspect", "Hillshade", "TRI", "TPI", "Roughness"]
    assert tuple(T.NAMES) == S.TERRAIN_PRODUCTS


def test_the_generator_is_deterministic_and_keeps_every_sum_exact():
    for seed in S.DEFAULT_SEEDS[:6]:
        a, b = S.build(seed), S.build(seed)
        assert a["ops"] == b["ops"] and a["specs"] == b["specs"] and a["grid"] == b["grid"] and a["plan"] == b["plan"]
        g = a["grid"]
        units = {"a": np.zeros(g["W"] * g["H"]), "b": np.zeros(g["W"] * g["H"])}
        for ca, cb in zip(a["clouds"], b["clouds"]):
            for k in ("x", "y", "a", "b", "t", "cls"):
                assert np.array_equal(ca[k], cb[k], equal_nan=True)
            assert np.array_equal(ca["a"] * 8, np.round(ca["a"] * 8)) and np.abs(ca["a"]).max(initial=0) <= 64
            assert np.array_equal(ca["b"], np.round(ca["b"])) and ca["b"].min(initial=0) >= 0 and ca["b"].max(initial=0) <= 4095
            cell = S.cells_of(g, ca["x"], ca["y"])
            m = cell >= 0
            units["a"] += np.bincount(cell[m], np.abs(ca["a"][m].astype(np.float64)) * 8, g["W"] * g["H"])
            units["b"] += np.bincount(cell[m], ca["b"][m].astype(np.float64), g["W"] * g["H"])
        assert max(units["a"].max(), units["b"].max()) < 1 << 24


def test_the_models_cells_are_the_oracles():
    """cells_of is the oracle's world_to_cell, point by point: the points on the bounds and a sample of the others."""
    for seed in S.DEFAULT_SEEDS[:8]:
        case = S.build(seed)
        g = case["grid"]
        og = O.make_grid((g["min_x"], g["min_y"], g["max_x"], g["max_y"]), cell=(g["cs"], -g["cs"]), tile=(g["tw"], g["th"]))
        assert (og.width, og.height) == (g["W"], g["H"])
        for c in case["clouds"]:
            n = len(c["x"])
            on_bounds = np.flatnonzero((c["x"] == g["min_x"]) | (c["x"] == g["max_x"]) | (c["y"] == g["min_y"]) | (c["y"] == g["max_y"]))
            pick = np.unique(np.concatenate([on_bounds[:200], np.arange(0, n, max(1, n // 300))])).astype(np.int64)
            cell = S.cells_of(g, c["x"], c["y"])
            for i in pick:
                col, row, ok = O.world_to_cell(og, float(c["x"][i]), float(c["y"][i]))
                assert cell[i] == (row * g["W"] + col if ok else -1), f"seed {seed}: point {i}"
