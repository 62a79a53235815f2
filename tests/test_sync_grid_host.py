"""The sync geometry grid, host side (no GPU): the input proof of tests/test_gpu_sync_grid.py and the
coverage the grid is there for.

1. On every window of tests/sync_grid_cases.py the oracle search (oracle/oracle_sync.cpp) finds the
   packet at the transmitted start with the packet's N_eff_TX, once, and nothing in the noise window.
2. The classes the cases reach, computed from the oracle's sync geometry alone: dropping or changing a
   case fails here, before a GPU is asked.
"""
import pytest

import oracle_py as O
import sync_grid_cases as G


@pytest.mark.parametrize("name", G.NAMES + [G.UNSUPPORTED_FOLLOWUP], ids=G.NAMES + ["after_the_refusal"])
def test_oracle_finds_every_packet(name):
    wins, starts = G.windows(name)
    refs = G.oracle_reports(name)
    _, chunk_len, S_win = G.recipe(name)
    g = O.sync_geometry(G.oracle_sync_cfg(name, chunk_len))
    psd, (_, _, n_ant, _, L, M) = G.case_def(name)
    # the search (in DECT-rate samples) and the fine search around its last coarse peak stay inside the window
    assert (g["search_len"] + g["D"] + g["stf_len"]) * L // M + g["xc_len"] + g["tmpl_len"] <= S_win, (name, g)
    assert len(wins) == G.N_PACKET_WINDOWS + 1 and all(w.shape == (n_ant, S_win) for w in wins)
    n_eff = O.packet_sizes(O.psdef(*psd))["N_eff_TX"]
    for w, start in enumerate(starts):
        assert [(o["fine_64"], o["N_eff_TX"]) for o in refs[w]] == [(start, n_eff)], (name, w, refs[w])
    assert refs[-1] == [], name


def _signature(name):
    """the sizes the launchers of kernels/sync_*.hip choose by: resampler class (L, M, os_min), step, patterns,
    fine FFT size, antennas"""
    g = G.sync_geometry(name)
    _, _, n_ant, os_min, L, M = G.CASES[name][1]
    return (L, M, os_min), g["step"], g["n_pattern"], G.log2_fft(g), n_ant


# one class per case and one case per class
CLASSES = {
    ((10, 9, 1), 8, 7, 9, 1),     # stream kernel <9, 10, 24, 0> at step 8, 512-point fine, n_uw 6
    ((10, 9, 1), 16, 7, 10, 1),   # ... at step 16
    ((10, 9, 1), 48, 9, 12, 1),   # ... at step 48 (sq 12), 9 patterns
    ((10, 9, 1), 48, 7, 11, 1),   # ... at step 48, 7 patterns, 2048-point
    ((10, 9, 1), 64, 7, 12, 1),   # pipe kernel with a 7-pattern STF
    ((1, 1, 1), 8, 7, 9, 1),      # <1, 1, 0>, 512-point, n_uw 6
    ((10, 9, 2), 96, 7, 12, 1),   # <9, 10, 4> at step 96, n_uw 6
    ((10, 9, 2), 96, 9, 13, 1),   # <9, 10, 4>, 8192-point fine, split rounds allowed
    ((10, 9, 2), 128, 9, 13, 2),  # step 128, D / 8 > 512, two antennas
    ((10, 9, 2), 128, 9, 13, 4),  # the same with four antennas
    ((40, 27, 1), 64, 9, 13, 1),  # <0, 0, 0> with 8192-point fine
}


def test_grid_covers_the_classes():
    sig = {name: _signature(name) for name in G.NAMES}
    assert len(set(sig.values())) == len(G.NAMES) == 11, sig
    assert set(sig.values()) == CLASSES, (set(sig.values()) ^ CLASSES)
    geo = {name: G.sync_geometry(name) for name in G.NAMES}
    steps = {g["step"] for g in geo.values()}
    assert {8, 16, 48, 96, 128} <= steps, steps
    assert any(g["n_pattern"] == 7 and g["step"] == 64 for g in geo.values())
    lgs = {G.log2_fft(g) for g in geo.values()}
    assert {9, 13} <= lgs, lgs
    assert any(g["D"] // 8 > 512 and G.CASES[name][1][2] > 1 for name, g in geo.items())
    # os2_C4 is the RX parity case of that name
    import phy_fixtures as F
    assert G.CASES["os2_C4"] == F.PARITY_CASES["os2_C4"][:2]
    # n_templates follows the context's antennas: 1, 2 and 3 templates are all searched
    assert {g["n_templates"] for g in geo.values()} >= {1, 2, 3}


def test_window_recipe():
    """the largest window is 51 712 samples x 4 antennas"""
    sizes = {name: (G.recipe(name)[2], G.CASES[name][1][2]) for name in G.NAMES}
    assert max(sizes.values()) == (51712, 4) == sizes["os2_C4"], sizes
    assert all(s % 2 == 0 for s, _ in sizes.values())
