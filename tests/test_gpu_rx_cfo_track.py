"""Residual CFO tracking from the DRS symbols on the GPU (dnrp_ctx_set_rx_cfo_tracking, dnrp_rx_cfo_track;
kernels/rx_drs.hip rx_cfo_track_kernel, the per-symbol mixer table through rx_fft_kernel, rx_fft_wave_kernel,
rx_fft_wave_ct_kernel and rx_epoch_kernel). Inputs, the numpy model and their proof against the injected
truth: tests/cfo_track_cases.py, tests/test_rx_cfo_track_host.py.

1. Default off, refused arguments; on -> off is a never-toggled context, LLRs and reports bit for bit.
2. gain 0 is the old receiver through the new plumbing: every processed table entry equals (n_stf inc0, inc1)
   bit for bit, LLRs byte-identical to off and at parity with the oracle, on the generic front end (10/9,
   os_min 2, 1/1, l mode), the wave front end (C3) and the epoch receiver / Y path at 4 x 4 (C4);
   rx_cfo_track ran, rx_fused did not although DNRP_RX_FUSED=1 asks for it.
3. gain 1 (and 0.5) on offset windows in L = M = 1 contexts: the device table against the model, the LLRs
   against the unchanged oracle on the input pre-rotated with the device's own table.
4. Benefit in l mode (case d): with tracking on the last quarter's PDC signs are the transmitted bits; off,
   the context reproduces the oracle's recorded error share.
5. The wave front end and the epoch receiver under an offset (C3 / C4 geometry, QPSK): the table against the
   injected truth within twice the model's deviation at the same b and omega, PDC signs against the
   transmitted bits, epoch receiver against Y path.
6. Continuation: a PCC batch of three offsets (omega, omega / 2, 0), the PDC call drops the middle one.
7. Both trackers on a drifted and offset window of case b: each table is the one of the run with only that
   tracker on, bit for bit.
8. Spatial multiplexing with tracking on is refused before any launch; the context stays usable.

TABLE_DIFF: the largest |device table - model table| measured on MI355X, as a fraction of one DRS period's
rotation (increments over one period's samples, and phases); the bound is ten times that (float pilot
products, summed in another order than numpy's) and never looser than TABLE_CAP = 1 % of a period.
"""
import numpy as np
import pytest

import cfo_track_cases as CT
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
TABLE_DIFF = {"a": 1.658e-07, "b": 9.735e-08, "c": 1.419e-08, "d": 4.703e-08, "a_half": 6.178e-08}
# measured |device - truth| / omega on MI355X, largest over the updates (C4: epoch receiver and Y path alike);
# recorded, the bound is twice cfo_track_cases.MODEL_DEV
TRUTH_DEV = {"C3": 0.0845, "C4": 0.0435}


def _table_bound(key):
    return TABLE_CAP if TABLE_DIFF[key] is None else min(TABLE_CAP, 10.0 * TABLE_DIFF[key])


def _rx(phy, psd, windows, reports, reqs, table=False, sto=False):
    """rx_run_helpers.rx as (PCC LLRs, PDC LLRs (torch, host), PCC reports, PDC reports, CFO table or None, STO
    table or None)"""
    r = H.rx(phy, psd, windows, reports, reqs, cfo_table=table, sto_table=sto)
    return r.pcc_llr, r.pdc_llr, r.rep1, r.rep2, r.cfo_tab, r.sto_tab


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
    assert fresh.rx_cfo_tracking() == (False, 1.0)
    with pytest.raises(dnrp.DnrpError) as e:
        fresh.rx_cfo_track(1)  # before any PCC call
    assert e.value.code == EINVAL
    a = _rx(fresh, psd, w, reports, reqs)
    with pytest.raises(dnrp.DnrpError) as e:
        fresh.rx_cfo_track(1)  # the PCC call ran with tracking off
    assert e.value.code == EINVAL
    assert fresh.kernel_time_total("rx_cfo_track")[1] == 0
    fresh.close()

    phy = _phy(ctx, lr)
    phy.set_rx_cfo_tracking(1, 0.5)
    assert phy.rx_cfo_tracking() == (True, 0.5)
    for on, gain in ((2, 1.0), (1, -0.25), (1, 1.5), (1, float("nan")), (1, float("inf"))):
        with pytest.raises(dnrp.DnrpError) as e:
            phy.set_rx_cfo_tracking(on, gain)
        assert e.value.code == EINVAL and phy.rx_cfo_tracking() == (True, 0.5)  # a refused call changes nothing
    assert phy.rx_sto_tracking() == (False, 1.0)  # the sister setting is its own
    phy.set_rx_cfo_tracking(0)
    assert phy.rx_cfo_tracking() == (False, 1.0)
    b = _rx(phy, psd, w, reports, reqs)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _same_reports(a[2], a[3], b[2], b[3])
    with pytest.raises(dnrp.DnrpError) as e:
        phy.rx_cfo_track(1)
    assert e.value.code == EINVAL
    assert phy.kernel_time_total("rx_cfo_track")[1] == 0
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
    on.set_rx_cfo_tracking(1, 0.0)
    b = _rx(on, psd, w, reports, reqs, table=True)
    counts = {k: on.kernel_time_total(k)[1] for k in ("rx_cfo_track", "rx_sto_track", "rx_fused", "rx_epoch", "rx_pdc")}
    on.close()
    ocf = O.cfg(phy_ctx[0], phy_ctx[1], phy_ctx[3], phy_ctx[4], phy_ctx[5])
    n_df, d = O.packet_sizes(O.psdef(*psd))["N_DF_symb"], O.dims(ocf, O.psdef(*psd))
    n_stf = d["STF_CP_os"] + d["N_b_DFT_os"]
    for i, _, _ in reqs:
        tab = b[4][i]
        assert np.all(np.isfinite(tab[0])), (tag, tab)
        assert np.all(tab[:n_df + 1].view(np.uint64) == tab[:1].view(np.uint64)), (tag, tab)  # (n_stf inc0, inc1)
        assert np.all(np.isnan(tab[n_df + 1:])), (tag, tab)
        cfo = float(reports[i].cfo_fractional_rad) + float(reports[i].cfo_integer_rad)
        assert abs(tab[0, 0] - n_stf * cfo) <= 1e-6 * n_stf, (tag, tab[0], cfo)
        assert abs(tab[0, 1] - float(b[2][i].cfo_fractional_rad) - float(reports[i].cfo_integer_rad)) <= 1e-6, (tag, tab[0])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), tag
    _same_reports(a[2], a[3], b[2], b[3])
    for r, (i, _, _) in enumerate(reqs):
        llr_gate.check((tag, "pcc"), b[0][i].numpy(), ref[r]["pcc_llr"])
        llr_gate.check((tag, "pdc"), b[1][r].numpy()[: len(ref[r]["pdc_llr"])], ref[r]["pdc_llr"])
    assert counts["rx_cfo_track"] > 0 and counts["rx_sto_track"] == 0 and counts["rx_fused"] == 0, (tag, counts)
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
def _offset(name, gain, monkeypatch, **env):
    """one offset packet of a case through a context with CFO tracking at `gain` (None: off)"""
    _clean_env(monkeypatch, **env)
    import dnrp
    g, w = CT.geometry(name), CT.window(name)
    phy = _phy(g["ctx"], g["lr"])
    if gain is not None:
        phy.set_rx_cfo_tracking(1, gain)
    rep = [dnrp.SyncReport(w["off"], 0.0, 0.0, g["psd"][0], g["psd"][1], g["sz"]["N_eff_TX"])]
    out = _rx(phy, g["psd"], [w["win"]], rep, [(0, w["nid"], w["pt"])], table=gain is not None)
    counts = {k: phy.kernel_time_total(k)[1] for k in ("rx_cfo_track", "rx_fused", "rx_epoch", "rx_pdc")}
    phy.close()
    return g, w, out, counts


@pytest.mark.parametrize("name,gain", [("a", 1.0), ("b", 1.0), ("c", 1.0), ("d", 1.0), ("a", 0.5)])
def test_table_and_llrs_under_offset(name, gain, monkeypatch):
    g, w, (pcc, pdc, rep1, _, tab, _), _ = _offset(name, gain, monkeypatch)
    tab = tab[0]
    n_df = g["N_DF"]
    assert np.all(np.isfinite(tab[:n_df + 1])) and np.all(np.isnan(tab[n_df + 1:]))
    a0, inc1 = tab[1]
    model = CT.model_table(g, w["win"], w["off"], a0, inc1, CT.inc_of_sto(g, rep1[0].sto_fractional), gain)
    diff = CT.table_diff(g, tab, model)
    key = name if gain == 1.0 else "a_half"
    print(f"cfo table {key}: device - model {diff:.3e} of a period's rotation, bound {_table_bound(key):.3e}; "
          f"device - truth {CT.model_deviation(g, tab, inc1):.4f} of omega")
    assert diff <= _table_bound(key), (key, diff)
    l0 = CT.updates(g)[0]
    assert tuple(tab[0]) == tuple(tab[l0]) and tab[l0 + 1, 1] != inc1  # a DRS symbol keeps the entry from before
    assert abs(tab[l0 + 1, 1] - (inc1 - gain * g["omega"])) <= CT.DEV_CAP * g["omega"]
    if gain != 1.0:
        return
    ref = O.rx(g["ocf"], g["ops"], CT.prerotate(g, w["win"], w["off"], tab), w["off"], 0.0, w["nid"], w["pt"])
    llr_gate.check((name, "pcc"), pcc[0].numpy(), ref["pcc_llr"])
    llr_gate.check((name, "pdc"), pdc[0].numpy()[: len(ref["pdc_llr"])], ref["pdc_llr"])


# ---------------------------------------------------------------- 4. benefit in l mode
def test_benefit_l_mode(monkeypatch):
    g, w, (_, pdc_on, _, _, tab, _), _ = _offset("d", 1.0, monkeypatch)
    G = g["sz"]["G"]
    bits = np.unpackbits(w["pdc"])[:G]
    q = slice(3 * G // 4, G)
    assert np.array_equal(bits[q], (pdc_on[0].numpy()[:G][q] > 0).astype(np.uint8))
    _, _, (_, pdc_off, _, _, _, _), counts = _offset("d", None, monkeypatch)
    assert counts["rx_cfo_track"] == 0
    ref = O.rx(g["ocf"], g["ops"], w["win"], w["off"], 0.0, w["nid"], w["pt"])
    llr_gate.check(("d", "off against the oracle"), pdc_off[0].numpy()[:G], ref["pdc_llr"])
    share = CT.last_quarter_errors(g, w, pdc_off[0].numpy())
    print(f"case d without tracking: {share:.4f} of the last quarter's PDC signs wrong (oracle {CT.BASELINE_D})")
    # the gate lets an LLR differ by one step, which flips a sign only at |LLR| <= 1: half a percent of the bits
    assert share >= CT.BASELINE_MIN and abs(share - CT.BASELINE_D) <= 0.005, share


# ---------------------------------------------------------------- 5. wave front end and epoch receiver under an offset
def _truth_and_signs(g, w, tab, pdc, tag):
    bound = 2.0 * CT.MODEL_DEV[CT.MODEL_OF[g["name"]]]
    dev = CT.model_deviation(g, tab, tab[1, 1])
    print(f"cfo table {tag}: device - truth {dev:.4f} of omega, bound {bound:.3f}")
    assert dev <= bound < CT.DEV_CAP, (tag, dev)
    G = g["sz"]["G"]
    assert np.array_equal(np.unpackbits(w["pdc"])[:G], (pdc[0].numpy()[:G] > 0).astype(np.uint8)), tag


def test_wave_front_end_under_offset(monkeypatch):
    g, w, (_, pdc, _, _, tab, _), counts = _offset("C3", 1.0, monkeypatch)
    assert counts["rx_cfo_track"] == 2 and counts["rx_epoch"] == 0, counts
    _truth_and_signs(g, w, tab[0], pdc, "C3")


def test_epoch_receiver_under_offset(monkeypatch):
    g, w, (pcc_e, pdc_e, _, _, tab_e, _), ce = _offset("C4", 1.0, monkeypatch, DNRP_RX_EPOCH="2")
    _, _, (pcc_y, pdc_y, _, _, tab_y, _), cy = _offset("C4", 1.0, monkeypatch, DNRP_RX_EPOCH="0")
    assert ce["rx_epoch"] > 0 and cy["rx_epoch"] == 0 and cy["rx_pdc"] > 0, (ce, cy)
    assert ce["rx_cfo_track"] == 2 and cy["rx_cfo_track"] == 2, (ce, cy)
    assert np.array_equal(tab_e, tab_y, equal_nan=True)
    _truth_and_signs(g, w, tab_e[0], pdc_e, "C4 epoch")
    _truth_and_signs(g, w, tab_y[0], pdc_y, "C4 ypath")
    assert torch.equal(pcc_e, pcc_y)  # the PCC phase is the same launches
    llr_gate.check(("C4", "epoch against ypath"), pdc_e[0].numpy(), pdc_y[0].numpy())


# ---------------------------------------------------------------- 6. continuation and selection
def test_continuation_and_selection(monkeypatch):
    import dnrp
    _clean_env(monkeypatch)
    g = CT.geometry("a")
    ws = [CT.window("a", omega=o, seed=s) for o, s in ((g["omega"], 3), (g["omega"] / 2, 4), (0.0, 5))]
    rep = lambda w: dnrp.SyncReport(w["off"], 0.0, 0.0, g["psd"][0], g["psd"][1], 1)
    phy = _phy(g["ctx"], g["lr"])
    phy.set_rx_cfo_tracking(1)
    reqs = [(2, ws[2]["nid"], ws[2]["pt"]), (0, ws[0]["nid"], ws[0]["pt"])]
    _, pdc3, _, _, tab3, _ = _rx(phy, g["psd"], [w["win"] for w in ws], [rep(w) for w in ws], reqs, table=True)
    # a second PDC call on the same PCC batch gives the same table
    _, pdc4, _, _, tab4, _ = _rx_pdc_again(phy, g["psd"], [w["win"] for w in ws], reqs)
    assert np.array_equal(tab3, tab4, equal_nan=True) and torch.equal(pdc3, pdc4)
    n_df = g["N_DF"]
    for row, i in ((1, 0), (0, 2)):
        _, pdc1, _, _, tab1, _ = _rx(phy, g["psd"], [ws[i]["win"]], [rep(ws[i])], [(0, ws[i]["nid"], ws[i]["pt"])], table=True)
        assert np.array_equal(tab3[i], tab1[0], equal_nan=True), i
        assert np.all(np.isfinite(tab3[i][:n_df + 1]))
        assert torch.equal(pdc3[row], pdc1[0]), i
    fin = np.isfinite(tab3[1][:, 1])
    p = int(np.argmin(fin))  # first NaN: pcc_max + 1
    assert 1 < p < n_df + 1 and np.all(fin[:p]) and not np.any(fin[p:]), tab3[1]
    assert np.all(np.isfinite(tab3[0][:p])) and np.array_equal(np.isfinite(tab3[0]), np.isfinite(tab3[2]))
    # the packet that ran both phases follows its offset; the one without an offset stays at the STF's increment
    assert abs(tab3[0][n_df, 1] - (tab3[0][1, 1] - g["omega"])) <= CT.DEV_CAP * g["omega"]
    period = g["step"] * g["sym"]
    assert np.max(np.abs(tab3[2][:n_df + 1, 1] - tab3[2][1, 1])) * period < 1e-3 * g["rot"]
    phy.close()


def _rx_pdc_again(phy, psd, windows, reqs):
    """the PDC batch once more on the PCC batch the context holds"""
    import dnrp
    ps = dnrp.psdef(*psd)
    sz = phy.packet_sizes(ps)
    n, n_rx, S = len(windows), phy.cfg.N_TX_max, windows[0].shape[1]
    dev = torch.device("cuda:0")
    iq = torch.from_numpy(np.stack(windows).view(np.float32).reshape(n, n_rx, S, 2)).to(dev)
    pdc_llr = torch.zeros((len(reqs), sz["G"]), dtype=torch.int16, device=dev)
    rep2 = phy.rx_pdc_batch([dnrp.PdcReq(ps, i, nid, pt) for i, nid, pt in reqs], iq, pdc_llr, want_report=True)
    phy.sync()
    return None, pdc_llr.cpu(), None, rep2, phy.rx_cfo_track(n), None


# ---------------------------------------------------------------- 7. both trackers
def test_both_trackers(monkeypatch):
    import dnrp
    _clean_env(monkeypatch)
    g = CT.geometry("b")
    w = CT.window("b", eps=ST.CASES["b"][3])
    rep = [dnrp.SyncReport(w["off"], 0.0, 0.0, g["psd"][0], g["psd"][1], g["sz"]["N_eff_TX"])]
    out = {}
    for key, sto, cfo in (("sto", 1, 0), ("cfo", 0, 1), ("both", 1, 1)):
        phy = _phy(g["ctx"], g["lr"])
        phy.set_rx_sto_tracking(sto)
        phy.set_rx_cfo_tracking(cfo)
        out[key] = _rx(phy, g["psd"], [w["win"]], rep, [(0, w["nid"], w["pt"])], table=bool(cfo), sto=bool(sto))
        counts = {k: phy.kernel_time_total(k)[1] for k in ("rx_sto_track", "rx_cfo_track")}
        assert counts == {"rx_sto_track": 2 * sto, "rx_cfo_track": 2 * cfo}, (key, counts)
        phy.close()
    n_df = g["N_DF"]
    assert np.array_equal(out["both"][4], out["cfo"][4], equal_nan=True)
    assert np.array_equal(out["both"][5], out["sto"][5], equal_nan=True)
    ctab, stab = out["both"][4][0], out["both"][5][0]
    assert abs(ctab[n_df, 1] - (ctab[1, 1] - g["omega"])) <= CT.DEV_CAP * g["omega"]  # each follows its own cause
    assert stab[n_df] != stab[0]


# ---------------------------------------------------------------- 8. spatial multiplexing
def test_spatial_multiplexing_is_refused(monkeypatch):
    import dnrp
    _clean_env(monkeypatch)
    psd_sm, ctx, _, _ = RG.CASES["sm22_256"]
    psd, ctx2, _, _ = RG.CASES["y21_256"]
    assert ctx == ctx2
    phy = _phy(ctx)
    phy.set_rx_mode(dnrp.Phy.RX_MODE_SM_MMSE)
    phy.set_rx_cfo_tracking(1, 0.0)
    w, reports, nids, types, _, _ = RG.windows("sm22_256")
    with pytest.raises(dnrp.DnrpError) as e:
        _rx(phy, psd_sm, w[:1], reports[:1], [(0, nids[0], types[0])])
    assert e.value.code == EUNSUPPORTED
    assert phy.kernel_time_total("rx_pdc")[1] == 0 and phy.kernel_time_total("rx_fft_pdc")[1] == 0  # nothing launched
    w, reports, nids, types, _, _ = RG.windows("y21_256")
    reqs = [(i, nids[i], types[i]) for i in range(len(w))]
    pcc, pdc, _, _, tab, _ = _rx(phy, psd, w, reports, reqs, table=True)
    phy.close()
    for i in range(len(w)):
        ref = RG.oracle("y21_256", i)
        llr_gate.check(("y21_256", i, "pcc"), pcc[i].numpy(), ref["pcc_llr"])
        llr_gate.check(("y21_256", i, "pdc"), pdc[i].numpy()[: len(ref["pdc_llr"])], ref["pdc_llr"])
        fin = np.isfinite(tab[i][:, 1])
        assert fin[0] and np.all(tab[i][fin] == tab[i][0])
