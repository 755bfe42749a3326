#!/usr/bin/env python3
"""Writes tests/golden/sequence_fuzz_cases.json: one SHA-256 per seed (sequence_fuzz_common.case_digest) of the 40 cases that
were the operation-sequence fuzz's suite before it drew terrain bands, recorded with the generator of that commit.

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
import sequence_fuzz_common as S  # noqa: E402

SEEDS = list(range(32)) + [47, 48, 49, 51, 54, 64, 75, 76]
OUT = os.path.join(HERE, "sequence_fuzz_cases.json")


def main():
    rec = {str(seed): S.case_digest(S.build(seed)) for seed in SEEDS}
    with open(OUT, "w") as f:
        json.dump(dict(what="sequence_fuzz_common.case_digest(build(seed)) per seed, before terrain was drawn", sha256=rec), f, indent=1)
        f.write("\n")
    print(f"{OUT}: {len(rec)} seeds")


if __name__ == "__main__":
    main()
