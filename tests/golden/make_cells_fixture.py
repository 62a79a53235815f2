"""Regenerate tests/golden/ref_cells.json from the reference's own compiled cell-map sources.

Builds oracle/_ref/ref_cells_harness (oracle/Makefile target `ref`: drs.cpp, pcc.cpp, pdc.cpp and
beamforming_and_antenna_port_mapping.cpp compiled unmodified from /root/reference, never shipped)
and condenses its JSON output into a committed fixture of data only. Run here only: the GPU box has
no /root/reference.

Layout of the fixture (normalise() below is the only writer; tests/test_cell_pins.py reads it
through expand helpers of its own and re-runs normalise() on fresh harness output where the
harness exists):

  L_MAX    symbols l = 1..L_MAX were walked after set_configuration(b, N_TS)
  tab      interned values, referenced by index from "cells": a list of uint32 (full index list,
           b <= 2), {"n": count, "sha": first 16 hex digits of the SHA-256 of the little-endian
           uint32 array} (b > 2), or a bit string (DRS values: '0' = +1, '1' = -1)
  cells    per (b, N_TS): pcc_symbol_idx_max; pcc = {"l": symbols, "k": tab index per symbol};
           drs = rows [l, ts_first, ts_last, [k tab index per stream], [y tab index per stream]];
           pdc = tab index of k_i_one_symbol for l = 1..L_MAX (an empty list where no PDC)
  counts   axes u, b, PLT, PL, N_eff_TX and nested arrays over the axes each value depends on;
           null where pdc.cpp asserts (N_eff_TX = 4 below 15 symbols, u = 8 with N_eff_TX = 8)
  W        per (N_TS, N_TX, codebook): matrix [N_TX][N_TS] as re, im pairs and both scalings
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_cells_harness")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_cells.json")
FULL_LISTS_B_MAX = 2

AXES = {"u": [1, 2, 4, 8], "b": [1, 2, 4, 8, 12, 16], "PLT": [0, 1], "PL": [1, 2, 3, 4, 8, 16],
        "N_eff_TX": [1, 2, 4, 8]}
# value name -> (column in a harness row, axes it depends on)
COUNT_COLS = {"N_PACKET_symb": (5, ("u", "PLT", "PL")), "N_DF_symb": (6, ("u", "PLT", "PL")),
              "N_DRS_symb_per_TS": (7, ("u", "PLT", "PL", "N_eff_TX")),
              "N_DRS_subc": (8, ("u", "b", "PLT", "PL", "N_eff_TX")),
              "N_PDC_subc": (9, ("u", "b", "PLT", "PL", "N_eff_TX")),
              "N_samples_DF": (10, ("u", "b", "PLT", "PL"))}
ROW_KEYS = ("u", "b", "PLT", "PL", "N_eff_TX")


def digest(values):
    """count + first 16 hex digits of the SHA-256 of the little-endian uint32 array"""
    a = np.asarray(values, dtype="<u4")
    return {"n": int(a.size), "sha": hashlib.sha256(a.tobytes()).hexdigest()[:16]}


def _nested(rows, col, axes):
    """rows -> nested lists over `axes`; every row that shares the axes' values must agree"""
    seen = {}
    for r in rows:
        key = tuple(r[ROW_KEYS.index(a)] for a in axes)
        v = None if r[col] < 0 else r[col]
        assert seen.setdefault(key, v) == v, (key, v, seen[key])

    def build(prefix, rest):
        if not rest:
            return seen[prefix]
        return [build(prefix + (x,), rest[1:]) for x in AXES[rest[0]]]
    return build((), axes)


def normalise(raw):
    tab, index = [], {}

    def intern(v):
        key = json.dumps(v, sort_keys=True)
        if key not in index:
            index[key] = len(tab)
            tab.append(v)
        return index[key]

    def cells(b, values):
        return intern(list(values) if b <= FULL_LISTS_B_MAX else digest(values))

    out = {"L_MAX": raw["L_MAX"], "cells": []}
    for g in raw["cells"]:
        b = g["b"]
        pcc_l = sorted({l for l, _ in g["pcc"]})
        assert [l for l, _ in g["pcc"]] == sorted(l for l, _ in g["pcc"]), "PCC symbols not ascending"
        drs = []
        for r in g["drs"]:
            ys = []
            for y in r["y"]:
                assert set(y) <= {"+", "-"}, "DRS value not +-1"
                ys.append(intern(y.replace("+", "0").replace("-", "1")))
            drs.append([r["l"], r["ts_first"], r["ts_last"], [cells(b, k) for k in r["k"]], ys])
        assert len(g["pdc"]) == raw["L_MAX"]
        out["cells"].append({
            "b": b, "N_TS": g["N_TS"], "pcc_symbol_idx_max": g["pcc_symbol_idx_max"],
            "pcc": {"l": pcc_l, "k": [cells(b, [k for l, k in g["pcc"] if l == s]) for s in pcc_l]},
            "drs": drs, "pdc": [cells(b, k) for k in g["pdc"]]})
    out["tab"] = tab
    rows = raw["counts"]
    assert len(rows) == int(np.prod([len(v) for v in AXES.values()]))
    out["counts"] = {"axes": AXES}
    for name, (col, axes) in COUNT_COLS.items():
        out["counts"][name] = {"axes": list(axes), "v": _nested(rows, col, axes)}
    out["W"] = raw["W"]
    return out


def dumps(data):
    return json.dumps(data, separators=(",", ":"), sort_keys=True) + "\n"


def run_harness():
    return json.loads(subprocess.run([HARNESS], check=True, capture_output=True, text=True).stdout)


def main() -> int:
    if not os.path.isdir("/root/reference"):
        print("reference not present; fixture left untouched")
        return 0
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
    text = dumps(normalise(run_harness()))
    with open(FIXTURE, "w") as f:
        f.write(text)
    print("wrote", FIXTURE, len(text), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
