"""The RX instantiation grid, host side (no GPU): the coverage tests/test_gpu_rx_grid.py is there for, and
the proof that its inputs are sound.

1. Every case's signature (receiver, N_RX, N_eff_TX, NBPS class) is computed from the oracle's packet_sizes
   and dims and from the context alone. Together with the older tables (PARITY_CASES, SM_CASES, EPOCH_CASES
   and the fused and Y-path lists of tests/test_gpu_parity.py) the signatures equal CLASSES, the literal set
   of every instantiation of launch_rx_epoch, launch_rx_fused, launch_rx_cells and launch_rx_cells_sm.
   Dropping a case fails here, before a GPU is asked.
2. The oracle demodulates every new window: at 20 dB and above (outside spatial multiplexing) the uncoded
   hard decisions stay below the error bound of _rx_parity, and the oracle's own float32 path stays inside
   llr_gate against its double path, so a float32 receiver can meet the gate on these windows.
"""
import numpy as np
import pytest

import llr_gate
import oracle_py as O
import phy_fixtures as F
import rx_grid_cases as G

dnrp = pytest.importorskip("dnrp")

PAIRS_EPOCH = [(1, 1), (2, 1), (4, 1), (2, 2), (4, 2), (4, 4)]                          # rx_epoch.hip epoch_pairs
PAIRS_ALL = [(1, 1), (2, 1), (4, 1), (8, 1), (2, 2), (4, 2), (8, 2), (4, 4), (8, 4)]    # fused_pairs, cells_pairs
PAIRS_SM = [(2, 2), (4, 2), (8, 2), (4, 4), (8, 4)]                                     # cells_sm_pairs

# every instantiation the four launchers can take: (receiver, N_RX, N_eff_TX, NBPS class)
CLASSES = (
    {("epoch", r, t, nb) for r, t in PAIRS_EPOCH for nb in (8, 0)}       # rx_epoch_kernel<R, T, NBPS>
    | {("fused", r, t, -1) for r, t in PAIRS_ALL}                        # rx_fused_kernel<R, T>
    | {("cells", r, t, nb) for r, t in PAIRS_ALL for nb in (8, 0)}       # rx_cells_kernel<R, T, false, NBPS>
    | {("cells_sm", r, t, nb) for r, t in PAIRS_SM for nb in (8, 6, 0)}  # rx_cells_kernel<R, T, true, NBPS>
)
# the Y path's wave front end (rx_fft_wave_ct_kernel) per antenna count
FRONT_CLASSES = {("wave_front", r) for r in (1, 2, 4, 8)}
# no instantiation is out of reach: every pair above has a valid packet and a context that fits the LDS
UNREACHABLE = set()


def _sig(psd, ctx, receiver):
    """the instantiation a run takes; receiver: "default" (DNRP_RX_EPOCH unset), "epoch" (=2), "fused",
    "ypath" (=0), "sm". Geometries outside the epoch and fused receivers run the cells kernel."""
    sz = O.packet_sizes(O.psdef(*psd))
    assert sz is not None, psd
    n_rx, t, sm = ctx[2], sz["N_eff_TX"], receiver == "sm"
    assert (sz["N_SS"] > 1) == sm, (psd, receiver)
    nb = G.nbps_class(sz["N_bps"], sm)
    wave = G.wave_geometry(psd, ctx)
    if sm:
        return ("cells_sm", n_rx, t, nb)
    if receiver == "fused" and wave and (n_rx, t) in PAIRS_ALL:
        return ("fused", n_rx, t, -1)
    if receiver in ("default", "epoch", "fused") and wave and (n_rx, t) in PAIRS_EPOCH and (receiver == "epoch" or n_rx >= 4):
        return ("epoch", n_rx, t, nb)
    return ("cells", n_rx, t, nb)


def _older_tables():
    """(table, name, signature) of every run of the tables of tests/test_gpu_parity.py"""
    import test_gpu_parity as P
    import inspect
    out = [("PARITY_CASES", n, _sig(c[0], c[1], "default")) for n, c in F.PARITY_CASES.items()]
    out += [("EPOCH_CASES", n, _sig(*F.PARITY_CASES[n][:2], "epoch")) for n in P.EPOCH_CASES]
    out += [("SM_CASES", n, _sig(c[0], c[1], "sm")) for n, c in P.SM_CASES.items()]
    lists = {}
    for fn in ("test_rx_parity_fused", "test_rx_parity_ypath"):
        mark = [m for m in getattr(P, fn).pytestmark if m.name == "parametrize"][0]
        lists[fn] = list(mark.args[1])
    out += [("fused", n, _sig(*F.PARITY_CASES[n][:2], "fused")) for n in lists["test_rx_parity_fused"]]
    out += [("ypath", n, _sig(*F.PARITY_CASES[n][:2], "ypath")) for n in lists["test_rx_parity_ypath"]]
    # test_rx_largest_cells_geometry: TM5 into 8 antennas at (8, 16), the default path
    src = inspect.getsource(P.test_rx_largest_cells_geometry)
    assert "((8, 16, 1, 1, 5, 8), (8, 16, 8, 1, 10, 9)" in src
    out.append(("largest_cells", "tm5_u8b16_rx8", _sig((8, 16, 1, 1, 5, 8), (8, 16, 8, 1, 10, 9), "default")))
    return out


def _new_runs():
    return [(name, rcv, _sig(G.CASES[name][0], G.CASES[name][1], rcv)) for name, rcv in G.RUNS]


def test_grid_covers_every_instantiation():
    older = {s for _, _, s in _older_tables()}
    new = {s for _, _, s in _new_runs()}
    assert older | new | UNREACHABLE == CLASSES, sorted((older | new | UNREACHABLE) ^ CLASSES)
    assert not UNREACHABLE & (older | new)
    # what the grid is there for: the instantiations no older table reaches, each by a named case
    missing_before = CLASSES - older
    assert missing_before <= new, sorted(missing_before - new)
    assert {("epoch", 4, 1, 8), ("epoch", 4, 1, 0), ("epoch", 4, 2, 8), ("epoch", 4, 2, 0), ("epoch", 4, 4, 0)} <= missing_before
    assert {("fused", r, t, -1) for r, t in PAIRS_ALL} - {("fused", 1, 1, -1), ("fused", 4, 4, -1)} <= missing_before
    # every run takes the receiver it is named for (no case passes on a fallback)
    want = {"epoch": "epoch", "fused": "fused", "ypath": "cells", "sm": "cells_sm"}
    for name, rcv, s in _new_runs():
        assert s[0] == want[rcv], (name, rcv, s)
    # the 4-antenna epoch cases run with DNRP_RX_EPOCH unset: the default path
    for name, rcv, s in _new_runs():
        if rcv == "epoch":
            assert ("DNRP_RX_EPOCH" not in G.env_of(name, rcv)) == (s[1] == 4), (name, s)
            assert _sig(G.CASES[name][0], G.CASES[name][1], "default" if s[1] == 4 else "epoch") == s
    # the generic epoch demapper sees every constellation below 256-QAM
    nbps = {O.packet_sizes(O.psdef(*G.CASES[n][0]))["N_bps"] for n, r, s in _new_runs() if r == "epoch" and s[3] == 0}
    assert nbps >= {1, 2, 4, 6}, nbps
    # the Y path's wave front end with every antenna count
    front = {("wave_front", c[1][2]) for _, c in F.PARITY_CASES.items() if G.wave_geometry(c[0], c[1]) and c[1][2] < 4}
    import test_gpu_parity as P
    mark = [m for m in P.test_rx_parity_ypath.pytestmark if m.name == "parametrize"][0]
    front |= {("wave_front", F.PARITY_CASES[n][1][2]) for n in mark.args[1] if G.wave_geometry(*F.PARITY_CASES[n][:2])}
    assert ("wave_front", 8) not in front
    front |= {("wave_front", G.CASES[n][1][2]) for n, r in G.RUNS if r == "ypath" and G.wave_geometry(*G.CASES[n][:2])}
    assert front >= {("wave_front", 1), ("wave_front", 4), ("wave_front", 8)}, front


def test_case_geometry():
    """the contexts and packets the issue of the grid sets: 1024 points at (u_max <= 2, 16) with the shortest
    valid packet of the mode, no u = 8; the cells-only cases at the smallest valid b; the epoch plan exists
    (rx_epoch_syms ok) for every epoch case in every mode and stride it runs with"""
    for name, (psd, ctx, snrs, rcvs) in G.CASES.items():
        u, b, plt, pl, tm, mcs = psd
        sz = O.packet_sizes(O.psdef(*psd))
        assert sz is not None and u <= 2 and ctx[0] == u and ctx[1] == b and sz["N_TX"] <= ctx[2], name
        shorter = [p for p in range(1, pl) if O.packet_sizes(O.psdef(u, b, plt, p, tm, mcs)) is not None]
        assert plt == 0 and not shorter, (name, shorter)
        if set(rcvs) & {"epoch", "fused"} or name.startswith("r8"):
            assert G.wave_geometry(psd, ctx) and b == 16, name
        else:
            smaller = [bb for bb in (1, 2, 4, 8, 12, 16) if bb < b
                       and O.packet_sizes(O.psdef(u, bb, plt, pl, tm, mcs)) is not None]
            assert not smaller, (name, smaller)
        assert 1 <= len(snrs) <= 2
    runs = [(n, 1, 2) for n, r in G.RUNS if r == "epoch"] + [(n, lr, st) for n, r, lr, st in G.VARIANTS if r == "epoch"]
    for name, lr, stride in runs:
        psd = G.CASES[name][0]
        sz = O.packet_sizes(O.psdef(*psd))
        ok = dnrp.query_table("rx_epoch_syms", psd[1], sz["N_TS"], sz["N_eff_TX"], sz["N_DF_symb"], lr, stride)[0]
        assert ok == 1, (name, lr, stride)
    for name, rcv, lr, stride in G.VARIANTS:
        assert (name, rcv) in G.RUNS and (lr, stride) in ((0, 2), (1, 3))
    assert {(r, lr, st) for _, r, lr, st in G.VARIANTS} == {(r, lr, st) for r in ("epoch", "fused", "ypath")
                                                            for lr, st in ((0, 2), (1, 3))}


def test_lds_fits():
    """the fused launch's LDS (N_RX wave regions) and the cells staging of the largest grid geometry fit one
    CU's 160 KiB: every fused and 8-antenna case is a parity case, none a refusal"""
    for n_rx in (1, 2, 4, 8):
        lds = int(dnrp.query_table("fused_lds_bytes", n_rx)[0])
        assert lds == n_rx * 9600 and lds <= 160 * 1024, (n_rx, lds)
    for name, (psd, ctx, _, _) in G.CASES.items():
        t = O.packet_sizes(O.psdef(*psd))["N_eff_TX"]
        lds = int(dnrp.query_table("cells_lds_bytes", ctx[0], ctx[1], psd[1], ctx[2], t)[0])
        assert lds <= 160 * 1024, (name, lds)


def _runs_of(name):
    """(lr, stride) pairs a case is demodulated with"""
    return sorted({(1, 2)} | {(lr, st) for n, _, lr, st in G.VARIANTS if n == name})


@pytest.mark.parametrize("name", G.NAMES)
def test_oracle_demodulates_every_window(name):
    psd, ctx, snrs, _ = G.CASES[name]
    sz = O.packet_sizes(O.psdef(*psd))
    w, reports, nids, types, pdc, _ = G.windows(name)
    assert len(w) == len(snrs) and all(x.shape == (ctx[2], O.dims(G.oracle_cfg(name), O.psdef(*psd))["N_packet_os_rs"]) for x in w)
    for lr, stride in _runs_of(name):
        for i, snr in enumerate(snrs):
            r = G.oracle(name, i, lr, stride)
            rf = G.oracle(name, i, lr, stride, use_float=True)
            assert len(r["pdc_llr"]) == sz["G"]
            bits = np.unpackbits(pdc[i])[: sz["G"]]
            ber = float(np.mean(bits != (r["pdc_llr"] > 0)))
            print(name, (lr, stride), i, snr, "uncoded BER", ber)
            if G.is_sm(name):
                if snr >= 30.0 and sz["N_bps"] <= 4:  # the bound of test_rx_sm_mmse_parity
                    assert ber < 5e-2, (name, i, ber)
            elif snr >= 20.0:                          # the bound of _rx_parity
                assert ber < 2e-2, (name, i, ber)
            llr_gate.check((name, lr, stride, i, "pcc", "float path"), rf["pcc_llr"], r["pcc_llr"])
            llr_gate.check((name, lr, stride, i, "pdc", "float path"), rf["pdc_llr"], r["pdc_llr"])
