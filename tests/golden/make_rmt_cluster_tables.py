#!/usr/bin/env python3
"""Extracts the vertex-clustering tables of the reference's isosurfacer into tests/golden/rmt_cluster_tables.json,
and its SHA-256 into rmt_cluster_tables.json.sha256.

Run where a checkout of the reference is at hand (the JSON is committed; nothing else needs the reference):
    FERREUS_REFERENCE=<reference checkout> python tests/golden/make_rmt_cluster_tables.py

Source (numbers only -- table VALUES are data, no source text is kept):
  * ferreus_rmt/src/constants.rs   NEIGHBOUR_MASKS (14 masks of 14 bits, Table 3), FLAT_HOLE_MASKS (36 pairs of masks,
                                   Table 4), ALL14_MASK

The product keeps its own copies (ferreus_rbf_rs_amd/csrc/isosurface.hpp, exported by bbfmm_isosurface_cluster_tables)
and tests/isosurface_cluster_restatement.py reads this file; tests/test_isosurface_cluster_host.py compares the two.
"""
import hashlib
import json
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))


def _const(src, name):
    m = re.search(r"pub const %s:\s*([^=]+?)=\s*(.*?);\n" % name, src, re.S)
    assert m, name
    return re.sub(r"//[^\n]*", "", m.group(2))


def _hex(text):
    return [int(t, 16) for t in re.findall(r"0x[0-9A-Fa-f]+", text)]


def parse(path):
    src = open(path).read()
    nb = _hex(_const(src, "NEIGHBOUR_MASKS"))
    fh = _hex(_const(src, "FLAT_HOLE_MASKS"))
    assert len(nb) == 14 and len(fh) == 72
    m = re.fullmatch(r"\s*\(1 << (\d+)\) - 1\s*", _const(src, "ALL14_MASK"))
    assert m
    return {"NEIGHBOUR_MASKS": nb, "FLAT_HOLE_MASKS": [fh[i:i + 2] for i in range(0, 72, 2)],
            "ALL14_MASK": (1 << int(m.group(1))) - 1}


def main():
    ref = os.environ.get("FERREUS_REFERENCE")
    if not ref:
        raise SystemExit("set FERREUS_REFERENCE to a checkout of the reference")
    tables = parse(os.path.join(ref, "ferreus_rmt", "src", "constants.rs"))
    tables["_source"] = "ferreus_rmt/src/constants.rs (values only)"
    out = os.path.join(HERE, "rmt_cluster_tables.json")
    text = json.dumps(tables, indent=1, sort_keys=True) + "\n"
    with open(out, "w") as f:
        f.write(text)
    with open(out + ".sha256", "w") as f:
        f.write(hashlib.sha256(text.encode()).hexdigest() + "  rmt_cluster_tables.json\n")
    print(out, {k: (len(v) if isinstance(v, list) else v) for k, v in tables.items() if not k.startswith("_")})


if __name__ == "__main__":
    main()
