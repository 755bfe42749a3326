#!/usr/bin/env python3
"""Writes tests/golden/sequence_fuzz_cases.json: one SHA-256 per seed (sequence_fuzz_common.case_digest) of the 40 cases that
were the operation-sequence fuzz's suite before it drew terrain bands, recorded with the generator of that commit, and under
the key `sha256_line` one per seed of LINE_SEEDS (the line cases: the digest covers the glyphs and the `dir` / `hl` arrays), and
under `sha256_acc` one per seed of ACC_SEEDS (the accumulator cases: the digest of the case as it is, its filters, `acc` lists,
trees, zonal and terrain lists and `z` arrays included), and under `sha256_poly` one per seed of POLY_SEEDS (the polygon cases:
the polygon sets' vertex bits and options, the uses, the point zonal entries, the new ops and the `lab` arrays too).

    python tests/golden/make_sequence_fuzz_cases.py

The digest leaves every plan's `terrain` list out, so tests/test_sequence_fuzz_host.py can hold a later generator to it: a seed
still means the same grid, reductions, filter, flavour, operations, clouds and marks.  Run it again only to ADD seeds; a digest
that changes for a seed already in the file means that the generator moved a draw.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))      # (a line case is thinned by the oracle)
import sequence_fuzz_common as S  # noqa: E402

SEEDS = list(range(32)) + [47, 48, 49, 51, 54, 64, 75, 76]
OUT = os.path.join(HERE, "sequence_fuzz_cases.json")


def main():
    def digest(seed):
        case = S.build(seed)
        for plan in [case["plan"]] + [o["plan"] for o in case["ops"] if o["op"] == "checkpoint" and o["plan"] is not None]:
            del plan["terrain"]
        return S.case_digest(case)

    rec = {str(seed): digest(seed) for seed in SEEDS}
    line = {str(seed): digest(seed) for seed in S.LINE_SEEDS}
    acc = {str(seed): S.case_digest(S.build(seed)) for seed in S.ACC_SEEDS}
    poly = {str(seed): S.case_digest(S.build(seed)) for seed in S.POLY_SEEDS}
    with open(OUT, "w") as f:
        json.dump(dict(what="sequence_fuzz_common.case_digest(build(seed)) per seed, before terrain was drawn", sha256=rec,
                       sha256_line=line, sha256_acc=acc, sha256_poly=poly), f, indent=1)
        f.write("\n")
    print(f"{OUT}: {len(rec)} + {len(line)} + {len(acc)} + {len(poly)} seeds")


if __name__ == "__main__":
    main()
