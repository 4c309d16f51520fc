#!/usr/bin/env python3
"""Extracts the curvature-weighting tables of the reference's isosurfacer into tests/golden/rmt_curvature_tables.json,
and its SHA-256 into rmt_curvature_tables.json.sha256.

Run where a checkout of the reference is at hand (the JSON is committed; nothing else needs the reference):
    FERREUS_REFERENCE=<reference checkout> python tests/golden/make_rmt_curvature_tables.py

Source (numbers only -- table VALUES are data, no source text is kept):
  * ferreus_rmt/src/constants.rs            rows 0..6 of NEIGHBOUR_EDGE_PLANE_PAIRS and NEIGHBOUR_EDGE_PLANE_PHIS (an
                                            owned edge has a label below 7; two or three planes of two edges each, the
                                            angles written out as numbers), PHI_1, PHI_2
  * ferreus_rmt/src/curvature_weighting.rs  EPS, MAX_COT_THETA, MAX_CURVATURE_WEIGHT

The product keeps its own copies (ferreus_rbf_rs_amd/csrc/isosurface_curvature.hpp, exported by
bbfmm_isosurface_curvature_tables) and tests/isosurface_curvature_restatement.py reads this file;
tests/test_isosurface_curvature_host.py compares the two.
"""
import hashlib
import json
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))


def _const(src, name):
    m = re.search(r"const %s:\s*([^=]+?)=\s*(.*?);\n" % name, src, re.S)
    assert m, name
    return re.sub(r"//[^\n]*", "", m.group(2))


def _rows(text):
    """The rows `&[[a, b], ...]` of a table as lists of pairs of tokens."""
    rows = re.findall(r"&\[((?:\s*\[[^\[\]]*\]\s*,?)+)\s*\]", text)
    return [[[t.strip() for t in pair.split(",")] for pair in re.findall(r"\[([^\[\]]*)\]", row)] for row in rows]


def parse(ref):
    consts = open(os.path.join(ref, "ferreus_rmt", "src", "constants.rs")).read()
    weighting = open(os.path.join(ref, "ferreus_rmt", "src", "curvature_weighting.rs")).read()
    phi = {n: float(_const(consts, n)) for n in ("PHI_1", "PHI_2")}
    pairs = [[[int(t) for t in pair] for pair in row] for row in _rows(_const(consts, "NEIGHBOUR_EDGE_PLANE_PAIRS"))]
    phis = [[[phi[t] for t in pair] for pair in row] for row in _rows(_const(consts, "NEIGHBOUR_EDGE_PLANE_PHIS"))]
    assert len(pairs) == 14 and len(phis) == 14 and all(len(a) == len(b) and len(a) in (2, 3) for a, b in zip(pairs, phis))
    out = {"NEIGHBOUR_EDGE_PLANE_PAIRS": pairs[:7], "NEIGHBOUR_EDGE_PLANE_PHIS": phis[:7], "PHI_1": phi["PHI_1"],
           "PHI_2": phi["PHI_2"]}
    for n in ("EPS", "MAX_COT_THETA", "MAX_CURVATURE_WEIGHT"):
        out[n] = float(_const(weighting, n))
    return out


def main():
    ref = os.environ.get("FERREUS_REFERENCE")
    if not ref:
        raise SystemExit("set FERREUS_REFERENCE to a checkout of the reference")
    tables = parse(ref)
    tables["_source"] = "ferreus_rmt/src/constants.rs, ferreus_rmt/src/curvature_weighting.rs (values only)"
    out = os.path.join(HERE, "rmt_curvature_tables.json")
    text = json.dumps(tables, indent=1, sort_keys=True) + "\n"
    with open(out, "w") as f:
        f.write(text)
    with open(out + ".sha256", "w") as f:
        f.write(hashlib.sha256(text.encode()).hexdigest() + "  rmt_curvature_tables.json\n")
    print(out, {k: (len(v) if isinstance(v, list) else v) for k, v in tables.items() if not k.startswith("_")})


if __name__ == "__main__":
    main()
