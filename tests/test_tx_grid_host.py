"""The TX form grid, host side (no GPU): the form choice of dnrp_tx_batch (host/tx.cpp plan_tx with
kernels/tx.hip tx_form_of) called through its host-only twin dnrp_tx_form_for for every case of TX_CASES, of
tests/test_gpu_tx_window.py and of tests/tx_grid_cases.py. The forms reached equal CLASSES, the literal set of
every branch of launch_tx; dropping a case fails here, before a GPU is asked. tests/test_gpu_tx_grid.py shows
on the device that a context's read-back (dnrp_tx_last_form) equals the twin.
"""
import pytest

import oracle_py as O
import phy_fixtures as F
import tx_grid_cases as G

dnrp = pytest.importorskip("dnrp")

RESAMPLERS = [(10, 9, 22), (10, 9, 4), (1, 1, 0), (0, 0, 0)]  # DNRP_TX_LAUNCH: os_min 1, os_min 2, 1/1, run-time ratio

# every branch of launch_tx
CLASSES = (
    {("stream", mode, q8, w) for mode in range(5) for q8 in (0, 1) for w in (0, 1)}   # DNRP_TXS x DNRP_TXS_W
    | {("wave", c, w) for c in RESAMPLERS for w in (0, 1)}                              # tx_kernel_wave<L, M, hl, w>
    | {("block", c, w) for c in RESAMPLERS for w in (0, 1)}                             # tx_kernel<L, M, hl, w>
    | {("scratch", 0), ("scratch", 1)}                                                  # tx_big_*: window kernel or not
    | {("wave", "unstaged"), ("block", "unstaged")}                                     # stage_bytes == 0
)
UNREACHABLE = set()  # a valid packet reaches every branch


def _older():
    import test_gpu_tx_window as W
    sig = {}
    for name, (psd, ctx, _, _, cb) in {**F.PARITY_CASES, **F.TX_ONLY_CASES}.items():
        sig[("TX_CASES", name)] = G.signature(dnrp.tx_form_for(ctx, dnrp.psdef(*psd), [cb] * G.N_PACKETS))
    for name, n, fraction, s_pad in G.OLDER_WINDOWED:
        psd, ctx = W.CONFIG[name]
        S = W.geometry(psd, ctx)["S"] + s_pad
        sig[("window", name, s_pad)] = G.signature(dnrp.tx_form_for(ctx, dnrp.psdef(*psd), [0] * n, S=S, win_fraction=fraction))
    return sig


def _new():
    sig = {(name, 0): G.signature(G.host_form(name)) for name in G.NAMES}
    sig.update({(name, 1): G.signature(G.host_form(name, windowed=True)) for name in G.WINDOWED})
    return sig


def test_grid_covers_every_form():
    older, new = set().union(*_older().values()), set().union(*_new().values())
    assert older | new | UNREACHABLE == CLASSES, sorted(map(str, (older | new | UNREACHABLE) ^ CLASSES))
    assert not UNREACHABLE & (older | new)
    # what the grid is there for
    assert {("wave", (10, 9, 22), 0), ("wave", (10, 9, 4), 0), ("wave", (10, 9, 4), 1), ("wave", (0, 0, 0), 0),
            ("wave", (0, 0, 0), 1), ("wave", "unstaged"), ("block", "unstaged"), ("stream", G.TXS_TXDIV, 0, 0),
            ("stream", G.TXS_TXDIV, 1, 0), ("stream", G.TXS_SM, 0, 0), ("stream", G.TXS_SM, 1, 0)} <= new - older
    assert ("wave", (10, 9, 22), 1) in older  # the odd row length of test_1024_point_wave_path_10_9


@pytest.mark.parametrize("name", G.NAMES)
def test_case_takes_its_form(name):
    psd, ctx, cb, misalign, want = G.CASES[name]
    sz = O.packet_sizes(O.psdef(*psd))
    assert sz is not None and psd[0] <= 2 and sz["N_TX"] <= ctx[2], name
    # the shortest valid packet of the mode -- or the shortest that takes the form
    assert psd[2] == 0
    for p in range(1, psd[3]):
        if O.packet_sizes(O.psdef(psd[0], psd[1], 0, p, psd[4], psd[5])) is not None:
            f = dnrp.tx_form_for(ctx, dnrp.psdef(psd[0], psd[1], 0, p, psd[4], psd[5]), [cb] * G.N_PACKETS, out_misalign=misalign)
            assert any(f[k] != v for k, v in want.items()), (name, p, f)
    for windowed in ([False, True] if name in G.WINDOWED else [False]):
        form = G.host_form(name, windowed)
        assert form["windowed"] == int(windowed)
        for k, v in want.items():
            assert form[k] == v, (name, windowed, k, form)
    form = G.host_form(name)
    if form["family"] == "stream":
        assert (form["L"], form["M"], form["hl"]) == (10, 9, 22) and form["n_seg"] >= 1 and 1 <= form["sb_chunks"] <= 4
        assert form["sb_chunks"] == 1 or form["mode"] in (G.TXS_SM, G.TXS_SM1)
        if form["mode"] == G.TXS_SISO and "bf" in name:
            assert sz["N_TS"] == 1 and sz["N_TX"] > 1
        if form["mode"] in (G.TXS_TXDIV, G.TXS_SM):  # W of the case's codebook is not a permutation
            w = dnrp.query_table("W", sz["N_TS"], sz["N_TX"], cb).reshape(sz["N_TX"], sz["N_TS"], 2)
            assert ((w != 0).any(axis=2).sum(axis=1) > 1).any(), name
    else:
        assert form["sb_chunks"] == form["n_seg"] == form["mode"] == form["q8"] == 0


def test_causes_of_the_wave_path():
    """each cause alone keeps a 10/9 packet at 1024 points off the streaming kernel"""
    import dnrp
    ctx, ps = (2, 16, 1, 1, 10, 9), dnrp.psdef(2, 16, 0, 1, 0, 1)
    S = dnrp.compute_packet_sizes(ps, 2, 16, 1, 10, 9)["N_samples_packet_os_rs"]
    assert dnrp.tx_form_for(ctx, ps, [0])["family"] == "stream"
    assert dnrp.tx_form_for(ctx, ps, [0], out_misalign=8)["family"] == "wave"      # iq_out not 16-byte aligned
    assert dnrp.tx_form_for(ctx, ps, [0], S=S + 1)["family"] == "wave"              # odd row length
    assert dnrp.tx_form_for((1, 16, 1, 1, 10, 9), dnrp.psdef(1, 16, 0, 1, 0, 1), [0])["family"] == "wave"  # 7 patterns
    # 8 spatial streams: 16-QAM fits the 4 KiB window, 64-QAM does not
    assert dnrp.tx_form_for((2, 16, 8, 1, 10, 9), dnrp.psdef(2, 16, 0, 2, 11, 3), [0])["sb_chunks"] == 4
    assert dnrp.tx_form_for((2, 16, 8, 1, 10, 9), dnrp.psdef(2, 16, 0, 2, 11, 5), [0])["family"] == "wave"
    # one packet with a codebook whose W is no permutation takes the whole batch off the one-hot form
    tm1 = dnrp.psdef(2, 16, 0, 1, 1, 3)
    assert dnrp.tx_form_for((2, 16, 2, 1, 10, 9), tm1, [0, 0, 0])["mode"] == G.TXS_TXDIV1
    assert dnrp.tx_form_for((2, 16, 2, 1, 10, 9), tm1, [0, 1, 0])["mode"] == G.TXS_TXDIV


def test_form_for_errors():
    import ctypes as C
    ps = dnrp.psdef(2, 16, 0, 1, 0, 1)
    with pytest.raises(dnrp.DnrpError) as e:  # S below the slot window
        dnrp.tx_form_for((2, 16, 1, 1, 10, 9), ps, [0], S=100)
    assert e.value.code == -1
    with pytest.raises(dnrp.DnrpError) as e:  # codebook out of range
        dnrp.tx_form_for((2, 16, 1, 1, 10, 9), ps, [7])
    assert e.value.code == -1
    with pytest.raises(dnrp.DnrpError) as e:  # u above the context's
        dnrp.tx_form_for((1, 16, 1, 1, 10, 9), ps, [0], S=1 << 20)
    assert e.value.code == -3
    with pytest.raises(dnrp.DnrpError) as e:  # N = 2 is the smallest window (64 / 8 * 0.1 rounds to 1)
        dnrp.tx_form_for((1, 1, 1, 1, 10, 9), dnrp.psdef(1, 1, 1, 1, 0, 1), [0], win_fraction=0.1)
    assert e.value.code == -1
    assert dnrp.lib().dnrp_tx_form_for(None, None, 0, None, 0, 0, C.c_float(0), None) == -1
    assert dnrp.lib().dnrp_tx_last_form(None, None) == -1
