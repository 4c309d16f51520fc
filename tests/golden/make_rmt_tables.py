#!/usr/bin/env python3
"""Extracts the marching-tetrahedra tables of the reference's isosurfacer into tests/golden/rmt_tables.json, and its
SHA-256 into rmt_tables.json.sha256.

Run where a checkout of the reference is at hand (the JSON is committed; nothing else needs the reference):
    FERREUS_REFERENCE=<reference checkout> python tests/golden/make_rmt_tables.py

Source (numbers only -- table VALUES are data, no source text is kept):
  * ferreus_rmt/src/constants.rs   EDGE_DELTAS (14 x 3), REVERSE_EDGE (14), OWNED_TET_EDGES (6 x 3),
                                   TET_EDGE_PAIRS (6 x 2), MT_TABLE (16 cases, 0..2 triangles of 3 tet-edge indices)

The product keeps its own copies (ferreus_rbf_rs_amd/csrc/isosurface.hpp, exported by bbfmm_isosurface_tables) and
tests/isosurface_restatement.py reads this file; tests/test_isosurface_host.py compares the two.
"""
import hashlib
import json
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))


def _ints(text):
    return [int(t) for t in re.findall(r"-?\d+", text)]


def _const(src, name):
    m = re.search(r"pub const %s:\s*([^=]+?)=\s*(.*?);\n" % name, src, re.S)
    assert m, name
    return m.group(2)


def parse(path):
    src = open(path).read()
    # drop line comments ("// 0" row labels) before reading numbers
    strip = lambda s: re.sub(r"//[^\n]*", "", s)
    ed = _ints(strip(_const(src, "EDGE_DELTAS")))
    rev = _ints(strip(_const(src, "REVERSE_EDGE")))
    tets = _ints(strip(_const(src, "OWNED_TET_EDGES")))
    pairs = _ints(strip(_const(src, "TET_EDGE_PAIRS")))
    assert len(ed) == 42 and len(rev) == 14 and len(tets) == 18 and len(pairs) == 12
    body = strip(_const(src, "MT_TABLE"))
    cases = re.findall(r"&\[(.*?)\],?\s*(?=&|\]$|$)", body.strip()[1:], re.S)
    mt = []
    for c in cases:
        nums = _ints(c)
        assert len(nums) % 3 == 0
        mt.append([nums[i:i + 3] for i in range(0, len(nums), 3)])
    assert len(mt) == 16, len(mt)
    return {
        "EDGE_DELTAS": [ed[i:i + 3] for i in range(0, 42, 3)],
        "REVERSE_EDGE": rev,
        "OWNED_TET_EDGES": [tets[i:i + 3] for i in range(0, 18, 3)],
        "TET_EDGE_PAIRS": [pairs[i:i + 2] for i in range(0, 12, 2)],
        "MT_TABLE": mt,
    }


def main():
    ref = os.environ.get("FERREUS_REFERENCE")
    if not ref:
        raise SystemExit("set FERREUS_REFERENCE to a checkout of the reference")
    tables = parse(os.path.join(ref, "ferreus_rmt", "src", "constants.rs"))
    tables["_source"] = "ferreus_rmt/src/constants.rs (values only)"
    out = os.path.join(HERE, "rmt_tables.json")
    text = json.dumps(tables, indent=1, sort_keys=True) + "\n"
    with open(out, "w") as f:
        f.write(text)
    with open(out + ".sha256", "w") as f:
        f.write(hashlib.sha256(text.encode()).hexdigest() + "  rmt_tables.json\n")
    print(out, {k: len(v) for k, v in tables.items() if not k.startswith("_")})


if __name__ == "__main__":
    main()
