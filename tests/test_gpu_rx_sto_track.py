"""Residual STO tracking from the DRS symbols on the GPU (dnrp_ctx_set_rx_sto_tracking, dnrp_rx_sto_track;
kernels/rx_drs.hip rx_sto_track_kernel, the per-symbol table through rx_fft_kernel, rx_fft_wave_kernel,
rx_fft_wave_ct_kernel and rx_epoch_kernel). Inputs, the numpy model and their proof against the injected
truth: tests/sto_track_cases.py, tests/test_rx_sto_track_host.py.

1. Default off; on -> off is a never-toggled context, LLRs and reports bit for bit.
2. gain 0 is the old receiver through the new plumbing: the table equals the STF increment bit for bit, LLRs
   byte-identical to off and at parity with the oracle, on the generic front end (10/9, os_min 2, 1/1, l mode),
   the wave front end (C3) and the epoch receiver / Y path at 4 x 4 (C4); rx_sto_track ran, rx_fused did not
   although DNRP_RX_FUSED=1 asks for it.
3. gain 1 (and 0.5) on drifted windows in L = M = 1 contexts: the device table against the model, the LLRs
   against the unchanged oracle on the input pre-rotated with the device's own table.
4. The wave front end and the epoch receiver under drift (C3 / C4 geometry, QPSK): the table against the
   injected truth within twice the model's deviation at the same b and eps, PDC signs against the
   transmitted bits, epoch receiver against Y path. Measured on MI355X: C3 0.060, C4 0.007 of a period.
5. Continuation: a PCC batch of three drifts, the PDC call drops the middle one.
6. Spatial multiplexing with tracking on is refused before any launch; the context stays usable.

TABLE_DIFF: the largest |device table - model table| measured on MI355X, as a fraction of one DRS period's
drift; the bound is ten times that (float pilot products, summed in another order than numpy's) and never
looser than TABLE_CAP = 1 % of a period.
"""
import numpy as np
import pytest

import llr_gate
import oracle_py as O
import phy_fixtures as F
import rx_grid_cases as RG
import rx_run_helpers as H
import sto_track_cases as ST
from rx_run_helpers import clean_env as _clean_env, phy as _phy

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
TABLE_CAP = 0.01
# measured |device - model| / period on the first MI355X run (case: value); see the module docstring
TABLE_DIFF = {"a": 1.025e-07, "b": 8.912e-08, "c": 2.374e-08, "d": 1.025e-07, "a_half": 4.342e-08}


def _table_bound(key):
    return TABLE_CAP if TABLE_DIFF[key] is None else min(TABLE_CAP, 10.0 * TABLE_DIFF[key])


def _rx(phy, psd, windows, reports, reqs, table=False):
    """rx_run_helpers.rx as (PCC LLRs, PDC LLRs (torch, host), PCC reports, PDC reports, table or None)"""
    r = H.rx(phy, psd, windows, reports, reqs, sto_table=table)
    return r.pcc_llr, r.pdc_llr, r.rep1, r.rep2, r.sto_tab


def _same_reports(a1, a2, b1, b2):
    H.same_pcc_reports(a1, b1)
    H.same_pdc_reports(a2, b2)


_PAR = {}


def _parity_case(name):
    """one packet of a PARITY_CASES geometry at the case's highest SNR, and the oracle's RX of it, computed once"""
    if name not in _PAR:
        psd, ctx, lr, snrs, cb = F.PARITY_CASES[name]
        u_max, b_max, n_rx, os_min, L, M = ctx
        ops, ocf = O.psdef(*psd), O.cfg(u_max, b_max, os_min, L, M, lr=lr)
        w, reports, nids, types, _, _ = RG.rx_windows(np.random.default_rng(11), ops, ocf, n_rx, (max(snrs),), cb)
        ref = O.rx(ocf, ops, w[0], reports[0].fine_peak_time, float(np.float32(reports[0].cfo_fractional_rad)),
                   nids[0], types[0])
        _PAR[name] = (psd, ctx, lr, w, reports, [(0, nids[0], types[0])], ref)
    return _PAR[name]


# ---------------------------------------------------------------- 1. default and toggle
@pytest.mark.parametrize("name", ["C2", "C3"])
def test_default_and_toggle(name, monkeypatch):
    import dnrp
    _clean_env(monkeypatch)
    psd, ctx, lr, w, reports, reqs, _ = _parity_case(name)
    fresh = _phy(ctx, lr)
    assert fresh.rx_sto_tracking() == (False, 1.0)
    with pytest.raises(dnrp.DnrpError) as e:
        fresh.rx_sto_track(1)  # before any PCC call
    assert e.value.code == EINVAL
    a = _rx(fresh, psd, w, reports, reqs)
    with pytest.raises(dnrp.DnrpError) as e:
        fresh.rx_sto_track(1)  # the PCC call ran with tracking off
    assert e.value.code == EINVAL
    assert fresh.kernel_time_total("rx_sto_track")[1] == 0
    fresh.close()

    phy = _phy(ctx, lr)
    phy.set_rx_sto_tracking(1, 0.5)
    assert phy.rx_sto_tracking() == (True, 0.5)
    for on, gain in ((2, 1.0), (1, -0.25), (1, 1.5), (1, float("nan")), (1, float("inf"))):
        with pytest.raises(dnrp.DnrpError) as e:
            phy.set_rx_sto_tracking(on, gain)
        assert e.value.code == EINVAL and phy.rx_sto_tracking() == (True, 0.5)  # a refused call changes nothing
    phy.set_rx_sto_tracking(0)
    assert phy.rx_sto_tracking() == (False, 1.0)
    b = _rx(phy, psd, w, reports, reqs)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _same_reports(a[2], a[3], b[2], b[3])
    with pytest.raises(dnrp.DnrpError) as e:
        phy.rx_sto_track(1)
    assert e.value.code == EINVAL
    phy.close()


# ---------------------------------------------------------------- 2. gain 0
GAIN0 = [("C2", None), ("os2", None), ("lm1_1_tm1", None), ("lmode_siso", None), ("C3", None), ("C4", "2"), ("C4", "0")]


def _gain0(phy_ctx, lr, psd, w, reports, reqs, ref, monkeypatch, epoch, tag):
    """off against on with gain 0 on one context configuration; returns the on context's launch counts"""
    env = {} if epoch is None else {"DNRP_RX_EPOCH": epoch}
    _clean_env(monkeypatch, **env)
    off = _phy(phy_ctx, lr)
    a = _rx(off, psd, w, reports, reqs)
    off.close()
    monkeypatch.setenv("DNRP_RX_FUSED", "1")  # asked for, and not taken while tracking is on
    on = _phy(phy_ctx, lr)
    on.set_rx_sto_tracking(1, 0.0)
    b = _rx(on, psd, w, reports, reqs, table=True)
    counts = {k: on.kernel_time_total(k)[1] for k in ("rx_sto_track", "rx_fused", "rx_epoch", "rx_pdc")}
    on.close()
    n_df = O.packet_sizes(O.psdef(*psd))["N_DF_symb"]
    for i, _, _ in reqs:
        tab = b[4][i]
        assert np.isfinite(tab[0]) and np.all(tab[:n_df + 1].view(np.uint64) == tab[:1].view(np.uint64)), (tag, tab)
        assert np.all(np.isnan(tab[n_df + 1:])), (tag, tab)
        nd = O.dims(O.cfg(phy_ctx[0], phy_ctx[1], phy_ctx[3], phy_ctx[4], phy_ctx[5]), O.psdef(*psd))["N_b_DFT_os"]
        assert abs(tab[0] - float(b[2][i].sto_fractional) * 2 * np.pi / nd) <= 1e-6 * max(1.0, abs(tab[0])), tag
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), tag
    _same_reports(a[2], a[3], b[2], b[3])
    for r, (i, _, _) in enumerate(reqs):
        llr_gate.check((tag, "pcc"), b[0][i].numpy(), ref[r]["pcc_llr"])
        llr_gate.check((tag, "pdc"), b[1][r].numpy()[: len(ref[r]["pdc_llr"])], ref[r]["pdc_llr"])
    assert counts["rx_sto_track"] > 0 and counts["rx_fused"] == 0, (tag, counts)
    return counts


@pytest.mark.parametrize("name,epoch", GAIN0, ids=[n if e is None else f"{n}-epoch{e}" for n, e in GAIN0])
def test_gain0_is_the_old_receiver(name, epoch, monkeypatch):
    psd, ctx, lr, w, reports, reqs, ref = _parity_case(name)
    counts = _gain0(ctx, lr, psd, w, reports, reqs, [ref], monkeypatch, epoch, (name, epoch))
    if epoch == "2":
        assert counts["rx_epoch"] > 0, counts
    if epoch == "0":
        assert counts["rx_epoch"] == 0 and counts["rx_pdc"] > 0, counts


# ---------------------------------------------------------------- 3. table against the model, LLRs against the oracle
def _drifted(name, gain, monkeypatch, **env):
    _clean_env(monkeypatch, **env)
    import dnrp
    g, w = ST.geometry(name), ST.window(name)
    phy = _phy(g["ctx"], g["lr"])
    phy.set_rx_sto_tracking(1, gain)
    rep = [dnrp.SyncReport(w["off"], 0.0, 0.0, g["psd"][0], g["psd"][1], g["sz"]["N_eff_TX"])]
    out = _rx(phy, g["psd"], [w["win"]], rep, [(0, w["nid"], w["pt"])], table=True)
    counts = {k: phy.kernel_time_total(k)[1] for k in ("rx_sto_track", "rx_fused", "rx_epoch", "rx_pdc")}
    phy.close()
    return g, w, out, counts


@pytest.mark.parametrize("name,gain", [("a", 1.0), ("b", 1.0), ("c", 1.0), ("d", 1.0), ("a", 0.5)])
def test_table_and_llrs_under_drift(name, gain, monkeypatch):
    g, w, (pcc, pdc, rep1, _, tab), _ = _drifted(name, gain, monkeypatch)
    tab = tab[0]
    n_df = g["N_DF"]
    assert np.all(np.isfinite(tab[:n_df + 1])) and np.all(np.isnan(tab[n_df + 1:]))
    model = ST.model_table(g, w["win"], w["off"], tab[0], float(rep1[0].cfo_fractional_rad), gain)
    diff = float(np.max(np.abs(tab[:n_df + 1] - model))) / ST.period_drift(g)
    key = name if gain == 1.0 else "a_half"
    print(f"sto table {key}: device - model {diff:.3e} of a period's drift, bound {_table_bound(key):.3e}; "
          f"device - truth {ST.model_deviation(g, tab):.4f}")
    assert diff <= _table_bound(key), (key, diff)
    assert tab[0] == tab[1] and tab[n_df] != tab[0]
    if gain != 1.0:
        return
    ref = O.rx(g["ocf"], g["ops"], ST.prerotate(g, w["win"], w["off"], tab), w["off"], 0.0, w["nid"], w["pt"])
    llr_gate.check((name, "pcc"), pcc[0].numpy(), ref["pcc_llr"])
    llr_gate.check((name, "pdc"), pdc[0].numpy()[: len(ref["pdc_llr"])], ref["pdc_llr"])


# ---------------------------------------------------------------- 4. wave front end and epoch receiver under drift
def _truth_and_signs(g, w, tab, pdc, tag):
    bound = 2.0 * ST.MODEL_DEV[ST.MODEL_OF[g["name"]]]
    dev = ST.model_deviation(g, tab)
    print(f"sto table {tag}: device - truth {dev:.4f} of a period's drift, bound {bound:.3f}")
    assert dev <= bound < ST.DEV_CAP, (tag, dev)
    G = g["sz"]["G"]
    assert np.array_equal(np.unpackbits(w["pdc"])[:G], (pdc[0].numpy()[:G] > 0).astype(np.uint8)), tag


def test_wave_front_end_under_drift(monkeypatch):
    g, w, (_, pdc, _, _, tab), counts = _drifted("C3", 1.0, monkeypatch)
    assert counts["rx_sto_track"] == 2 and counts["rx_epoch"] == 0, counts
    _truth_and_signs(g, w, tab[0], pdc, "C3")


def test_epoch_receiver_under_drift(monkeypatch):
    g, w, (pcc_e, pdc_e, _, _, tab_e), ce = _drifted("C4", 1.0, monkeypatch, DNRP_RX_EPOCH="2")
    _, _, (pcc_y, pdc_y, _, _, tab_y), cy = _drifted("C4", 1.0, monkeypatch, DNRP_RX_EPOCH="0")
    assert ce["rx_epoch"] > 0 and cy["rx_epoch"] == 0 and cy["rx_pdc"] > 0, (ce, cy)
    assert np.array_equal(tab_e, tab_y, equal_nan=True)
    _truth_and_signs(g, w, tab_e[0], pdc_e, "C4 epoch")
    _truth_and_signs(g, w, tab_y[0], pdc_y, "C4 ypath")
    assert torch.equal(pcc_e, pcc_y)  # the PCC phase is the same launches
    llr_gate.check(("C4", "epoch against ypath"), pdc_e[0].numpy(), pdc_y[0].numpy())


# ---------------------------------------------------------------- 5. continuation and selection
def test_continuation_and_selection(monkeypatch):
    import dnrp
    _clean_env(monkeypatch)
    g = ST.geometry("a")
    ws = [ST.window("a", eps=e, seed=s) for e, s in ((1.0e-3, 3), (5.0e-4, 4), (0.0, 5))]
    rep = lambda w: dnrp.SyncReport(w["off"], 0.0, 0.0, g["psd"][0], g["psd"][1], 1)
    phy = _phy(g["ctx"], g["lr"])
    phy.set_rx_sto_tracking(1)
    _, pdc3, _, _, tab3 = _rx(phy, g["psd"], [w["win"] for w in ws], [rep(w) for w in ws],
                              [(2, ws[2]["nid"], ws[2]["pt"]), (0, ws[0]["nid"], ws[0]["pt"])], table=True)
    n_df = g["N_DF"]
    for row, i in ((1, 0), (0, 2)):
        _, pdc1, _, _, tab1 = _rx(phy, g["psd"], [ws[i]["win"]], [rep(ws[i])], [(0, ws[i]["nid"], ws[i]["pt"])], table=True)
        assert np.array_equal(tab3[i], tab1[0], equal_nan=True), i
        assert np.all(np.isfinite(tab3[i][:n_df + 1]))
        assert torch.equal(pdc3[row], pdc1[0]), i
    fin = np.isfinite(tab3[1])
    p = int(np.argmin(fin))  # first NaN: pcc_max + 1
    assert 1 < p < n_df + 1 and np.all(fin[:p]) and not np.any(fin[p:]), tab3[1]
    assert np.all(np.isfinite(tab3[0][:p])) and np.array_equal(np.isfinite(tab3[0]), np.isfinite(tab3[2]))
    assert np.max(np.abs(tab3[2][:n_df + 1] - tab3[2][0])) < 1e-3 * ST.period_drift(g)  # the packet without drift
    phy.close()


# ---------------------------------------------------------------- 6. spatial multiplexing
def test_spatial_multiplexing_is_refused(monkeypatch):
    import dnrp
    _clean_env(monkeypatch)
    psd_sm, ctx, _, _ = RG.CASES["sm22_256"]
    psd, ctx2, _, _ = RG.CASES["y21_256"]
    assert ctx == ctx2
    phy = _phy(ctx)
    phy.set_rx_mode(dnrp.Phy.RX_MODE_SM_MMSE)
    phy.set_rx_sto_tracking(1, 0.0)
    w, reports, nids, types, _, _ = RG.windows("sm22_256")
    with pytest.raises(dnrp.DnrpError) as e:
        _rx(phy, psd_sm, w[:1], reports[:1], [(0, nids[0], types[0])])
    assert e.value.code == EUNSUPPORTED
    assert phy.kernel_time_total("rx_pdc")[1] == 0 and phy.kernel_time_total("rx_fft_pdc")[1] == 0  # nothing launched
    w, reports, nids, types, _, _ = RG.windows("y21_256")
    reqs = [(i, nids[i], types[i]) for i in range(len(w))]
    pcc, pdc, _, _, tab = _rx(phy, psd, w, reports, reqs, table=True)
    phy.close()
    for i in range(len(w)):
        ref = RG.oracle("y21_256", i)
        llr_gate.check(("y21_256", i, "pcc"), pcc[i].numpy(), ref["pcc_llr"])
        llr_gate.check(("y21_256", i, "pdc"), pdc[i].numpy()[: len(ref["pdc_llr"])], ref["pdc_llr"])
        assert np.isfinite(tab[i][0]) and np.all(tab[i][np.isfinite(tab[i])] == tab[i][0])
