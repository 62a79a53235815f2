"""Reader of tests/golden/ref_cells.json (TEST INFRASTRUCTURE): the DRS / PCC / PDC cells, packet
counts and beamforming matrices as the reference's compiled drs.cpp, pcc.cpp, pdc.cpp and W_t
produce them (oracle/ref_cells_harness.cpp, condensed by tests/golden/make_cells_fixture.py, which
documents the layout). Shared by tests/test_cell_pins.py and tests/test_gpu_cell_grid.py."""
import hashlib
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_cells.json")
GOLD = json.load(open(PATH))
TAB = GOLD["tab"]
L_MAX = GOLD["L_MAX"]
GEOMETRIES = [(g["b"], g["N_TS"]) for g in GOLD["cells"]]
_BY_GEOMETRY = {(g["b"], g["N_TS"]): g for g in GOLD["cells"]}


def geometry(b, N_TS):
    return _BY_GEOMETRY[(b, N_TS)]


def digest(values):
    a = np.asarray(values, dtype="<u4")
    return {"n": int(a.size), "sha": hashlib.sha256(a.tobytes()).hexdigest()[:16]}


def count(idx):
    """number of cells of tab entry idx (a full list or a count + digest)"""
    e = TAB[idx]
    return len(e) if isinstance(e, list) else e["n"]


def matches(idx, values):
    """values (ints) equal tab entry idx: the list where the fixture has one, else count + digest"""
    e, v = TAB[idx], [int(x) for x in values]
    return v == e if isinstance(e, list) else digest(v) == e


def full_list(idx):
    """the index list of tab entry idx, None where the fixture holds only its digest"""
    e = TAB[idx]
    return list(e) if isinstance(e, list) else None


def bits(idx):
    """DRS values of tab entry idx as +-1 floats ('0' = +1, '1' = -1)"""
    return np.array([1.0 if c == "0" else -1.0 for c in TAB[idx]])


def counts(name):
    """{axes tuple: value} of a counts table, in the order of its own axes"""
    t, axes = GOLD["counts"][name], GOLD["counts"]["axes"]
    out = {}

    def walk(v, prefix, rest):
        if not rest:
            out[prefix] = v
            return
        for x, sub in zip(axes[rest[0]], v):
            walk(sub, prefix + (x,), rest[1:])
    walk(t["v"], (), t["axes"])
    return t["axes"], out
