"""The operation-sequence fuzz (tests/sequence_fuzz_common.py) on the HOST engine (ExecutionMode.CPU), and what it rests on.

The existing suites hold the host engine to the oracle, so where the model and the host engine disagree the model is wrong: this
run pins the model on a machine without a GPU, before tests/test_gpu_sequence_fuzz.py holds the HIP engine to it.  The host
engine hands out no plane or flag pointers and has one flavour; the runner drops those ops, the generator draws them all the same
-- test_the_default_seeds_cover_the_situations looks at what was drawn.

Line cases (seeds from LINE_SEED_BASE on; LINE_SEEDS in the suite) append Line-glyph reductions and a Point WeightedAverage to
what a seed draws: their sums are exact too (a visit has weight 1), so the model -- the oracle's footprint, added in binary64 --
needs no tolerance.  Gaussian groups are not drawn: their weights are expf values and their sums depend on the order of
addition.  _line_pass checks the exactness condition for the Line sums with the oracle's binary64 mode; the test of the
generator below checks it again.

Accumulator cases (seeds from ACC_SEED_BASE on; ACC_SEEDS in the suite) add a float32 channel `z`, surface channels, per-reduction
filters, histograms, extremes, cell stats, tree bands and zonal tables to what a seed draws, in core: integer states and
bit-defined bands, so the model -- the *_common models of each feature, from the same routing -- needs no tolerance either.

Polygon cases (seeds from POLY_SEED_BASE on; POLY_SEEDS in the suite) are the accumulator case of seed - POLY_SEED_BASE +
ACC_SEED_BASE with polygon channels, point zonal entries, polygon-burnt zones and outlines on top: set_polygons between ingests
(also right behind an ingest_async nobody waited for), point_zonal read anywhere, set_zones from a polygon set, polygonize under
zonal's freshness rule, and zones burnt back from the crowns' outlines.  The models are the features' own brute-force ones
(points_in_polygons_common, point_zonal_common, rasterize_common, polygonize_common): everything bit for bit again."""
import json
import os

import numpy as np
import pytest

import pcr
import pcr_oracle_py as O
import sequence_fuzz_common as S
import terrain_common as T
from conftest import GOLDEN


@pytest.mark.parametrize("seed", S.DEFAULT_SEEDS + S.LINE_SEEDS + S.ACC_SEEDS + S.POLY_SEEDS)
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


def test_the_line_seeds_cover_the_line_situations():
    """Every situation the line cases are for occurs in at least three of LINE_SEEDS, recognised from the case alone; no seed
    of the list is idle, and what a line case is holds for each."""
    assert all(seed >= S.LINE_SEED_BASE for seed in S.LINE_SEEDS) and max(S.DEFAULT_SEEDS) < S.LINE_SEED_BASE
    assert S.seeds_from_env("PCR_SEQ_FUZZ_NO_SUCH_VARIABLE") == S.DEFAULT_SEEDS + S.LINE_SEEDS + S.ACC_SEEDS + S.POLY_SEEDS
    seen = {name: [] for name in S.LINE_SITUATIONS}
    for seed in S.LINE_SEEDS:
        case = S.build(seed)
        assert case["line"] and case["ops"][-1]["op"] == "finalize" and 4 <= len(case["ops"]) <= 12, seed
        lines = [s for s in case["specs"] if "glyph" in s]
        assert 1 <= len(lines) <= 4 and case["specs"][-len(lines):] == lines and len(case["specs"]) <= 15, seed
        assert all(s["type"] in S.LINE_TYPES and s["glyph"]["maxr"] in S.LINE_MAX_RADIUS for s in lines), seed
        assert 1 <= len({tuple(sorted(s["glyph"].items())) for s in lines}) <= 2, seed
        assert all(gr["glyph"] is None or set(gr["slots"]) <= {0, 1} for gr in case["groups"]), seed
        found = S.situations(case)
        assert found <= set(S.SITUATIONS) | set(S.LINE_SITUATIONS)
        for name in found & set(S.LINE_SITUATIONS):
            seen[name].append(seed)
    for name in S.LINE_SITUATIONS:
        assert len(seen[name]) >= 3, f"'{name}' occurs in seeds {seen[name]} only"
    for seed in S.LINE_SEEDS:                                     # the smallest list: no seed can go
        rest = [s for s in S.LINE_SEEDS if s != seed]
        assert any(sum(s in seen[name] for s in rest) < 3 for name in S.LINE_SITUATIONS), f"seed {seed} adds nothing"
    assert not any(S.build(seed)["line"] for seed in S.DEFAULT_SEEDS[:3])


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


def test_the_line_seeds_are_the_cases_they_were():
    """... and LINE_SEEDS are pinned the same way under a key of their own: the digest of a line case covers the glyphs of its
    specs and the `dir` / `hl` arrays of its clouds."""
    with open(os.path.join(GOLDEN, "sequence_fuzz_cases.json")) as f:
        want = json.load(f)["sha256_line"]
    assert sorted(int(s) for s in want) == sorted(S.LINE_SEEDS)
    for seed in S.LINE_SEEDS:
        case = S.build(seed)
        for plan in [case["plan"]] + [o["plan"] for o in case["ops"] if o["op"] == "checkpoint" and o["plan"] is not None]:
            del plan["terrain"]
        assert S.case_digest(case) == want[str(seed)], f"line seed {seed} is another case than it was"


def test_the_accumulator_seeds_cover_the_accumulator_situations():
    """Every situation the accumulator cases are for occurs in at least three of ACC_SEEDS, recognised from the case alone; and
    what an accumulator case is holds for each: in core, never a line case, at least one accumulator entry, filters within
    create's limits, `z` on every cloud without a +0.0, every cell far below the counters' wrap points."""
    assert all(seed >= S.ACC_SEED_BASE for seed in S.ACC_SEEDS) and max(S.LINE_SEEDS) < S.ACC_SEED_BASE
    assert 15 <= len(S.ACC_SEEDS) <= 30 and len(set(S.ACC_SEEDS)) == len(S.ACC_SEEDS)
    assert not S.build(S.LINE_SEEDS[0])["acc"] and not S.build(0)["acc"]
    seen = {name: [] for name in S.ACC_SITUATIONS}
    kinds = set()
    for seed in S.ACC_SEEDS:
        case = S.build(seed)
        acc, plan = case["acc"], case["plan"]
        assert acc is not None and not case["line"] and not case["flavour"]["ooc"] and case["ops"][-1]["op"] == "finalize", seed
        assert not case["marked"] and not case["split_first"], seed
        entries = S.acc_entries(acc)
        assert 1 <= len(entries) <= 9 and max(len(acc[k]) for k in ("hist", "ext", "stats")) <= 3, seed
        assert len(acc["surfaces"]) <= 2 and len(plan["trees"]) <= 2 and len(plan["zonal"]) <= 2, seed
        filters = {S.filter_key(e["filt"]) for e in entries + case["specs"] if e["filt"]}
        assert len(filters) <= 8 and all(len(f) <= 3 for f in filters), seed
        assert all(s["ch"] in ("a", "b") for s in case["specs"] if s["type"] in ("Sum", "Count", "Average", "WeightedAverage")), seed
        assert all(h["bins"] in S.HIST_BINS and h["bins"] * case["grid"]["W"] * case["grid"]["H"] <= S.ACC_MAX_COUNTERS for h in acc["hist"]), seed
        assert all(e["k"] in S.EXT_K and e["gap"] in S.EXT_GAPS for e in acc["ext"]), seed
        assert all((s["origin"], s["res"]) in S.STAT_STEPS and 1 <= len(set(s["products"])) == len(s["products"]) <= 3 for s in acc["stats"]), seed
        names = [S.band_name(i, s) for i, s in enumerate(case["specs"])] + [n for n, _, _, _ in S.acc_bands(acc)]
        assert len(set(names)) == len(names), seed
        assert all(t["source"] in names + ["dtm", "hag"] for t in plan["trees"] + plan["terrain"]), seed
        assert sum(len(c["x"]) for c in case["clouds"]) < 1 << 22, seed           # N below 2^32, S2 exact below 2^22 points a cell
        for c in case["clouds"]:
            assert c["z"].dtype == np.float32 and len(c["z"]) == len(c["x"]) and not (c["z"].view(np.uint32) == 0).any(), seed
            kinds.add(c["shape"])
        assert all(o["plan"] is None and o["flavour"] is None for o in case["ops"] if o["op"] == "checkpoint"), seed
        found = S.situations(case)
        assert found <= set(S.ACC_SITUATIONS)
        for name in found:
            seen[name].append(seed)
    for name in S.ACC_SITUATIONS:
        assert len(seen[name]) >= 3, f"'{name}' occurs in seeds {seen[name]} only"
    assert {"hot_acc", "entry_filtered", "pipeline_filtered", "empty"} <= kinds, kinds


def test_the_accumulator_seeds_are_the_cases_they_are():
    """ACC_SEEDS are pinned under a key of their own: the digest of an accumulator case covers the filters of its specs, the
    `acc` lists, the plan's trees, zonal and terrain lists, the inserted ops and the `z` arrays of its clouds."""
    with open(os.path.join(GOLDEN, "sequence_fuzz_cases.json")) as f:
        want = json.load(f)["sha256_acc"]
    assert sorted(int(s) for s in want) == sorted(S.ACC_SEEDS)
    for seed in S.ACC_SEEDS:
        a, b = S.build(seed), S.build(seed)
        assert S.case_digest(a) == S.case_digest(b) == want[str(seed)], f"accumulator seed {seed} is another case than it was"
        z = np.concatenate([c["z"] for c in a["clouds"]])
        if len(z) < 5000:                                         # (a case of a few points need not hold every kind)
            continue
        assert np.isnan(z).any() and np.isposinf(z).any() and np.isneginf(z).any() and (z.view(np.uint32) == 0x80000000).any(), seed
        assert ((z.view(np.uint32) & 0x7F800000) == 0).sum() > (z.view(np.uint32) == 0x80000000).sum(), seed      # denormals
        assert (np.abs(z[np.isfinite(z)]) > 1e5).any(), seed                       # beyond every [lo, hi) and +-2^21 steps


def test_the_polygon_seeds_cover_the_polygon_situations():
    """Every situation the polygon cases are for occurs in at least three of POLY_SEEDS, recognised from the case alone; no seed
    of the list is idle; and what a polygon case is holds for each: the accumulator case of its seed underneath, 1 to 3 polygon
    channels of 1 or 2 sets below POLY_MAX_EDGES edges, 1 to 3 point zonal entries within create's limits, points outside the
    grid and inside a polygon in every cloud that has points to spare, checkpoints refused."""
    import points_in_polygons_common as PIP
    assert all(seed >= S.POLY_SEED_BASE for seed in S.POLY_SEEDS) and max(S.ACC_SEEDS) < S.POLY_SEED_BASE
    assert 12 <= len(S.POLY_SEEDS) <= 24 and len(set(S.POLY_SEEDS)) == len(S.POLY_SEEDS)
    seen = {name: [] for name in S.POLY_SITUATIONS}
    op_kinds, label_kinds, set_kinds = set(), set(), set()
    for seed in S.POLY_SEEDS:
        case = S.build(seed)
        base = S.build(seed - S.POLY_SEED_BASE + S.ACC_SEED_BASE)
        po, acc, plan, g = case["poly"], case["acc"], case["plan"], case["grid"]
        assert po is not None and acc is not None and not case["line"] and not case["flavour"]["ooc"] and case["ops"][-1]["op"] == "finalize", seed
        # the accumulator case underneath: the grid, the plan's drawn parts, the ops it had in their order, the specs it had
        assert case["grid"] == base["grid"] and case["fwfi"] == base["fwfi"] and case["path"] == base["path"] and case["filt"] == base["filt"], seed
        new_ops = ("set_polygons", "point_tables", "set_zones_poly", "polygonize", "reburn")
        strip = lambda o: {k: v for k, v in o.items() if k not in ("group", "sync")}
        assert [strip(o) for o in case["ops"] if o["op"] not in new_ops] == [strip(o) for o in base["ops"]], seed
        assert [(s["type"], s["ch"]) for s in case["specs"][:len(base["specs"])]] == [(s["type"], s["ch"]) for s in base["specs"]], seed
        assert plan["terrain"] == base["plan"]["terrain"] and plan["trees"] == base["plan"]["trees"], seed
        assert 1 <= len(po["names"]) <= 3 and po["names"] == list(S.POLY_NAMES[:len(po["names"])]), seed
        for sets in po["sets"]:
            assert 1 <= len(sets) <= 2, seed
            for st in sets + po["zone_sets"]:
                assert len(st["polys"].coords) <= S.POLY_MAX_EDGES and st["polys"].P >= 1, seed
                assert (st["opts"]["index_cols"], st["opts"]["index_rows"]) in PIP.INDEX_SIZES, seed
                set_kinds.update(st["opts"]["kinds"])
        assert all(st["opts"]["rect"] is not None for st in po["sets"][0]), seed
        assert 1 <= len(po["pz"]) <= 3 and len(acc["hist"]) <= 4 and len(plan["zonal"]) <= 4, seed
        for e in po["pz"]:
            assert e["max_zones"] in S.PZ_MAX_ZONES and 1 <= len(e["stats"]) + len(e["hists"]) <= 4, seed
            assert len({s["ch"] for s in e["stats"]}) == len(e["stats"]) and len({h["ch"] for h in e["hists"]}) == len(e["hists"]), seed
            assert all((s["origin"], s["res"]) in S.STAT_STEPS for s in e["stats"]), seed
            assert all((h["lo"], h["hi"]) in S.HIST_RANGES and h["bins"] in S.HIST_BINS for h in e["hists"]), seed
            label_kinds.add("polygon" if e["label"] in po["names"] else "surface" if e["label"] in [sc["name"] for sc in acc["surfaces"]] else e["label"])
        filters = {S.filter_key(e["filt"]) for e in S.acc_entries(acc) + case["specs"] + [s for e in po["pz"] for s in e["stats"] + e["hists"]]
                   if e["filt"]}
        assert len(filters) <= 8 and sum(len(f) for f in filters) + (1 if case["filt"] else 0) + len(po["clip"]) <= 32, seed
        assert all(s["ch"] in ("a", "b") for s in case["specs"] if s["type"] in ("Sum", "Average", "WeightedAverage")), seed
        assert sum(len(c["x"]) for c in case["clouds"]) < 1 << 22, seed
        assert S.point_units(g, case["clouds"]).max() + S.PATCH_UNITS * sum(o["op"] == "planes_write" for o in case["ops"]) < 1 << 24, seed
        for i, k, cur in S.poly_walk(case):
            c = case["clouds"][k]
            assert ("lab" in c) == any(e["label"] == "lab" for e in po["pz"]) and S.cloud_keys(c)[:7] == S.CLOUD_KEYS + S.ACC_CLOUD_KEYS, seed
            if len(c["x"]) >= 2000 and c["shape"] != "pipeline_emptied":     # a share outside the grid and inside a polygon
                ch = S.poly_channels(case, k, cur)
                out = S.cells_of(g, c["x"], c["y"]) < 0
                assert any((out & (S.zones_of(v) > 0)).any() or (out & (v != np.float32(st[j]["opts"]["background"])) & ~np.isnan(v)).any()
                           for (name, v), st, j in zip(ch.items(), po["sets"], cur)), (seed, k)
        assert all(o["plan"] is None and o["flavour"] is None for o in case["ops"] if o["op"] == "checkpoint"), seed
        op_kinds.update(o["op"] for o in case["ops"])
        found = S.situations(case)
        assert found <= set(S.POLY_SITUATIONS)
        for name in found:
            seen[name].append(seed)
    for name in S.POLY_SITUATIONS:
        assert len(seen[name]) >= 3, f"'{name}' occurs in seeds {seen[name]} only"
    for seed in S.POLY_SEEDS:                                     # no seed of the list is idle
        rest = [s for s in S.POLY_SEEDS if s != seed]
        assert any(sum(s in seen[name] for s in rest) < 3 for name in S.POLY_SITUATIONS), f"seed {seed} adds nothing"
    assert {"set_polygons", "point_tables", "set_zones_poly", "polygonize", "reburn", "checkpoint"} <= op_kinds, op_kinds
    assert {"polygon", "surface", "cls", "lab"} <= label_kinds, label_kinds
    assert {"partition", "donut", "ngons", "rect"} <= set_kinds and any(k.startswith("degenerate") for k in set_kinds), set_kinds


def test_the_polygon_seeds_are_the_cases_they_are():
    """POLY_SEEDS are pinned under a key of their own: the digest of a polygon case covers the polygon sets (vertex bits) and
    their options, the uses, the point zonal entries, the inserted ops and the `lab` arrays.  Two builds are one case."""
    with open(os.path.join(GOLDEN, "sequence_fuzz_cases.json")) as f:
        want = json.load(f)["sha256_poly"]
    assert sorted(int(s) for s in want) == sorted(S.POLY_SEEDS)
    for seed in S.POLY_SEEDS:
        a, b = S.build(seed), S.build(seed)
        assert S.case_digest(a) == S.case_digest(b) == want[str(seed)], f"polygon seed {seed} is another case than it was"
    # the digest sees a vertex, an option, an entry and a label
    a = S.build(S.POLY_SEEDS[0])
    d0 = S.case_digest(a)
    a["poly"]["sets"][0][0]["polys"].coords[0, 0] = np.nextafter(a["poly"]["sets"][0][0]["polys"].coords[0, 0], np.inf)
    d1 = S.case_digest(a)
    a["poly"]["sets"][0][0]["opts"]["index_cols"] += 1
    d2 = S.case_digest(a)
    a["poly"]["pz"][0]["max_zones"] += 1
    d3 = S.case_digest(a)
    assert len({d0, d1, d2, d3}) == 4


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


def test_the_generator_is_deterministic_for_line_seeds_and_keeps_every_line_sum_exact():
    """Two builds of a line seed are one case, `dir` and `hl` included; the channels are what the draw promises; and per Line
    group and cell the sum of |v| over every visit of every cloud, from the oracle in its binary64 mode, stays below 2^24
    units with every plane patch of the case added (units of 1/8 on `a`, of 1 on `b`)."""
    for seed in S.LINE_SEEDS[:6]:
        a, b = S.build(seed), S.build(seed)
        assert a["ops"] == b["ops"] and a["specs"] == b["specs"] and a["grid"] == b["grid"] and a["plan"] == b["plan"]
        assert S.case_digest(a) == S.case_digest(b)
        g = a["grid"]
        og = S.oracle_grid(g)
        lines = [gr for gr in a["groups"] if gr["glyph"] is not None]
        units = [np.zeros((g["H"], g["W"])) for _ in lines]
        for ca, cb in zip(a["clouds"], b["clouds"]):
            assert S.cloud_keys(ca) == S.CLOUD_KEYS + S.LINE_CLOUD_KEYS
            for k in S.cloud_keys(ca):
                assert np.array_equal(ca[k], cb[k], equal_nan=True) and len(ca[k]) == len(ca["x"])
            assert ca["dir"].dtype == ca["hl"].dtype == np.float32 and np.isfinite(ca["dir"]).all() and np.isfinite(ca["hl"]).all()
            assert np.abs(ca["dir"]).max(initial=0) <= 80 and np.abs(ca["hl"]).max(initial=0) <= S.LINE_LONG_CELLS * g["cs"]
            assert np.array_equal(ca["a"] * 8, np.round(ca["a"] * 8)) and np.abs(ca["a"]).max(initial=0) <= 64
            assert np.array_equal(ca["b"], np.round(ca["b"])) and ca["b"].min(initial=0) >= 0 and ca["b"].max(initial=0) <= 4095
            inside = S.cells_of(g, ca["x"], ca["y"]) >= 0
            if not inside.any():
                continue
            mag = {"a": np.abs(ca["a"]) * np.float32(8), "b": ca["b"]}
            for u, gr in zip(units, lines):
                u += np.nan_to_num(S.oracle_line(og, gr["glyph"], O.SUM, ca, mag[gr["ch"]], inside, wide=True)).astype(np.float64)
        patched = S.PATCH_UNITS * sum(o["op"] == "planes_write" for o in a["ops"])
        assert max(u.max() for u in units) + patched < 1 << 24, seed
        # ... and the Point groups' sums, from the clouds as the line pass left them (it replaces some)
        assert S.point_units(g, a["clouds"]).max() + patched < 1 << 24, seed


def test_the_models_line_footprint_and_touched_tiles_are_the_oracles():
    """Cloud by cloud on six line seeds.  What carries weight: the tiles Model.ingest flags -- the centre cells' tiles, by
    cells_of -- are the tiles the oracle touched, and the oracle's Sum band is a number exactly in the flagged tiles (the
    footprint is clipped to them, Q4: no visit leaves a flagged tile, none lands in another).  The comparison of the planes
    themselves only pins the model's plumbing (filter, channels, NaN -> 0, which plane): both sides are the same oracle, so it
    is no independent check of the footprint -- the oracle is the footprint, held to the reference by its own tests."""
    for seed in S.LINE_SEEDS[:6]:
        case = S.build(seed)
        g = case["grid"]
        og = S.oracle_grid(g)
        for c in case["clouds"]:
            model = S.Model(case)
            model.ingest(c)
            sel = S.keep_mask(case["filt"], c["cls"])
            for gr, pl in zip(case["groups"], model.planes):
                if gr["glyph"] is None:
                    continue
                ogl = O.make_glyph(O.GLYPH_LINE, half_length=gr["glyph"]["hl"], max_radius=gr["glyph"]["maxr"])
                kw = dict(half_length=c["hl"][sel]) if gr["glyph"]["hl_ch"] else {}
                red = {p: O.Reduction(og, rtype, ogl) for p, rtype in ((0, O.SUM), (1, O.COUNT)) if p in gr["slots"]}
                for p, r in red.items():
                    r.ingest(c["x"][sel], c["y"][sel], c[gr["ch"]][sel], direction=c["dir"][sel], **kw)
                    band = r.finalize()
                    assert np.array_equal(np.nan_to_num(band).reshape(-1), pl[p]), f"seed {seed}: plane {p} of a {c['shape']} cloud"
                    touched = np.array([[r.tile_touched(tr, tc) for tc in range(model.tx)] for tr in range(model.ty)])
                    assert np.array_equal(touched, model.touched), f"seed {seed}: touched tiles of a {c['shape']} cloud"
                    if p == 0:
                        assert np.array_equal(~np.isnan(band).reshape(-1), model.touched_cells()), f"seed {seed}: NaN mask"
                    r.close()
