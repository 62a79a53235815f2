"""Angle-of-arrival report from the DRS pilots on the GPU (dnrp_ctx_set_rx_aoa, dnrp_rx_aoa; kernels/rx_drs.hip
rx_aoa_kernel<2 | 4 | 8> at the end of every PDC path but the fused one). Cases, the numpy restatement and the
pilot model: tests/aoa_cases.py; their proof on the CPU: tests/test_rx_aoa_host.py.

1. Noiseless, every case: || R / tr R - a a^H / N_RX ||_F <= 1e-4 (rank one whatever the front end does; the float
   pilots carry about 1e-6 relative error), az_rad within the CPU-measured interpolation bias + 1e-4 rad of the
   truth, peak >= 1 - 1e-3, n_cells from the oracle's DRS cells, Hermitian symmetry exact, and the launches each
   case is there for (rx_epoch and rx_aoa; the plain Y path without rx_fused; the trackers; the MMSE receiver).
2. Noisy L = M = 1 cases: || R - R_model ||_F <= 1e-4 tr R_model, the model fed the device's PCC report.
3. Every case: az_rad, peak and grid_idx equal the numpy restatement and dnrp.aoa_estimate fed the device's own R
   (index exact, 1e-6 rad / 1e-6).
4. Off is free: LLRs, reports and rx_mimo_detail rows byte-identical on and off, no launch and DNRP_ESTATE while
   off, setter / getter round trip, refusals, a new setting holds from the next PDC call, m = 0, and two runs of
   one call give bit-identical rows.

Measured on MI355X (printed by the tests): see OBSERVED.
"""
import numpy as np
import pytest

import aoa_cases as AC
import rx_run_helpers as H
from rx_run_helpers import clean_env as _clean_env, phy as _phy

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -7
RANK_ONE_BOUND, MODEL_BOUND = 1e-4, 1e-4
# the largest figures of the first MI355X run: item 1's rank-one distance (sm42; 6.2e-9 for ula2), item 2's
# distance from the model (ula4_td; 1.2e-7 for ula2), both far below 1e-5, the level above which a cause would have to be found before accepting the figure
OBSERVED = {"rank_one": 4.3e-8, "model": 2.4e-7}
TIMERS = ("rx_aoa", "rx_epoch", "rx_fused", "rx_pdc", "rx_sto_track", "rx_cfo_track")

_RUN = {}


def _reports(g, ws):
    import dnrp
    return [dnrp.SyncReport(w["off"], 0.0, 0.0, g["psd"][0], g["psd"][1], g["sz"]["N_eff_TX"]) for w in ws]


def _context(g):
    import dnrp
    phy = _phy(g["ctx"])
    if g["sm"]:
        phy.set_rx_mode(dnrp.Phy.RX_MODE_SM_MMSE)
    if g["track"]:
        phy.set_rx_sto_tracking(1)
        phy.set_rx_cfo_tracking(1)
    return phy


def _run(name, snr_db, monkeypatch):
    """one PCC and one PDC call of a case with the report on, computed once: (geometry, windows, requests'
    window indices, rows, PCC reports, launch counts)"""
    key = (name, snr_db)
    if key not in _RUN:
        g, ws = AC.geometry(name), AC.windows(name, snr_db)
        _clean_env(monkeypatch, **g["env"])
        phy = _context(g)
        phy.set_rx_aoa(g["pos"], *g["scan"])
        reqs = [(i, ws[i]["nid"], ws[i]["pt"]) for i in g["req"]]
        r = H.rx(phy, g["psd"], [w["win"] for w in ws], _reports(g, ws), reqs)
        rows = phy.rx_aoa(len(reqs))
        counts = {k: phy.kernel_time_total(k)[1] for k in TIMERS}
        phy.close()
        _RUN[key] = (g, ws, list(g["req"]), rows, r.rep1, counts)
    return _RUN[key]


ALL = list(AC.CASES)
NOISY = [(n, AC.NOISY_SNR_DB) for n in AC.MODEL_CASES]


# ---------------------------------------------------------------- 1. noiseless
@pytest.mark.parametrize("name", ALL)
def test_noiseless_rank_one(name, monkeypatch):
    g, ws, idx, rows, _, counts = _run(name, None, monkeypatch)
    n = g["n_rx"]
    for r, i in enumerate(idx):
        R8 = rows["R"][r]
        R = R8[:n, :n].astype(np.complex128)
        a = AC.steering(g["pos"], np.deg2rad(ws[i]["az_deg"]))
        tr = np.trace(R).real
        d = float(np.linalg.norm(R / tr - np.outer(a, a.conj()) / n))
        err = AC.ang_err_deg(rows["az_rad"][r], ws[i]["az_deg"])
        print(f"aoa noiseless {name} row {r}: rank-one distance {d:.3e}, az error {err:.5f} deg, peak {rows['peak'][r]:.7f}")
        assert d <= RANK_ONE_BOUND, (name, r, d)
        assert err <= AC.BIAS_DEG[AC.bias_kind(name)] + np.rad2deg(1e-4), (name, r, err)
        assert rows["peak"][r] >= 1.0 - 1e-3
        assert rows["n_cells"][r] == g["n_cells"]
        assert np.array_equal(R8, R8.conj().T) and np.all(R8.diagonal().imag == 0.0)
        assert not np.any(R8[n:, :]) and not np.any(R8[:, n:]) and not np.any(rows["reserved"][r])
    assert counts["rx_aoa"] > 0 and counts["rx_fused"] == 0, counts
    if name == "c4":
        assert counts["rx_epoch"] > 0, counts
    if name == "c4_y":
        assert counts["rx_epoch"] == 0 and counts["rx_pdc"] > 0, counts
    if g["track"]:
        assert counts["rx_sto_track"] > 0 and counts["rx_cfo_track"] > 0, counts


# ---------------------------------------------------------------- 2. noisy, against the pilot model
@pytest.mark.parametrize("name", AC.MODEL_CASES)
def test_noisy_covariance_equals_model(name, monkeypatch):
    g, ws, idx, rows, rep1, _ = _run(name, AC.NOISY_SNR_DB, monkeypatch)
    n = g["n_rx"]
    for r, i in enumerate(idx):
        model = AC.model_cov(g, ws[i]["win"], ws[i]["off"], float(rep1[i].cfo_fractional_rad))
        R = rows["R"][r][:n, :n].astype(np.complex128)
        d = float(np.linalg.norm(R - model) / np.trace(model).real)
        err = AC.ang_err_deg(rows["az_rad"][r], ws[i]["az_deg"])
        print(f"aoa noisy {name} row {r}: |R - model| / tr {d:.3e}, az error {err:.3f} deg")
        assert d <= MODEL_BOUND, (name, r, d)
        assert err <= 2.0 * AC.NOISY_ERR_DEG[name] + np.rad2deg(1e-4), (name, r, err)


# ---------------------------------------------------------------- 3. the scan against the restatement and the twin
@pytest.mark.parametrize("name,snr", [(n, None) for n in ALL] + NOISY, ids=lambda v: "noiseless" if v is None else str(v))
def test_scan_equals_restatement_and_twin(name, snr, monkeypatch):
    import dnrp
    g, _, idx, rows, _, _ = _run(name, snr, monkeypatch)
    for r in range(len(idx)):
        R = rows["R"][r]
        ref = AC.estimate(g["pos"], *g["scan"], R, g["n_rx"])
        twin = dnrp.aoa_estimate(g["pos"], *g["scan"], R, g["n_rx"])
        for what, e in (("restatement", (ref["grid_idx"], ref["az_rad"], ref["peak"], ref["lag"])),
                        ("twin", (twin["grid_idx"], twin["az_rad"], twin["peak"], twin["lag"]))):
            assert rows["grid_idx"][r] == e[0], (name, r, what)
            assert abs(float(rows["az_rad"][r]) - e[1]) <= 1e-6, (name, r, what)
            assert abs(float(rows["peak"][r]) - e[2]) <= 1e-6, (name, r, what)
            assert abs(complex(rows["lag"][r]) - e[3]) <= 1e-6 * max(1.0, abs(e[3])), (name, r, what)


# ---------------------------------------------------------------- 4. off is free, the interface
@pytest.mark.parametrize("name", ["ula4_td", "c4"])
def test_off_is_free(name, monkeypatch):
    import dnrp
    g, ws = AC.geometry(name), AC.windows(name, AC.NOISY_SNR_DB if name in AC.MODEL_CASES else None)
    _clean_env(monkeypatch, **g["env"])
    reqs = [(i, ws[i]["nid"], ws[i]["pt"]) for i in g["req"]]
    wins, reports = [w["win"] for w in ws], _reports(g, ws)
    off = _context(g)
    off.set_rx_mimo_report(detail=1)
    assert off.rx_aoa_cfg() is None
    a = H.rx(off, g["psd"], wins, reports, reqs, detail=True)
    assert off.kernel_time_total("rx_aoa")[1] == 0
    with pytest.raises(dnrp.DnrpError) as e:
        off.rx_aoa(1)
    assert e.value.code == ESTATE
    off.close()
    on = _context(g)
    on.set_rx_mimo_report(detail=1)
    on.set_rx_aoa(g["pos"], *g["scan"])
    b = H.rx(on, g["psd"], wins, reports, reqs, detail=True)
    rows = on.rx_aoa(len(reqs))
    assert on.kernel_time_total("rx_aoa")[1] > 0
    assert torch.equal(a.pcc_llr, b.pcc_llr) and torch.equal(a.pdc_llr, b.pdc_llr)
    H.same_pcc_reports(a.rep1, b.rep1)
    H.same_pdc_reports(a.rep2, b.rep2)
    assert a.rows.tobytes() == b.rows.tobytes()
    # two runs of one call: bit-identical rows
    H.rx(on, g["psd"], wins, reports, reqs)
    assert on.rx_aoa(len(reqs)).tobytes() == rows.tobytes()
    with pytest.raises(dnrp.DnrpError) as e:
        on.rx_aoa(len(reqs) + 1)
    assert e.value.code == EINVAL
    # on -> off: no launch, no rows
    on.set_rx_aoa(None)
    assert on.rx_aoa_cfg() is None
    on.kernel_time_total("rx_aoa")
    c = H.rx(on, g["psd"], wins, reports, reqs)
    assert on.kernel_time_total("rx_aoa")[1] == 0 and torch.equal(a.pdc_llr, c.pdc_llr)
    with pytest.raises(dnrp.DnrpError) as e:
        on.rx_aoa(1)
    assert e.value.code == ESTATE
    on.close()


def test_setting_round_trip_and_refusals(monkeypatch):
    import dnrp
    _clean_env(monkeypatch)
    phy = _phy((1, 1, 4, 2, 1, 1))
    pos, scan = AC.uca(4, 0.35), (-1.0, 2.0, 64)
    phy.set_rx_aoa(pos, *scan)
    got = phy.rx_aoa_cfg()
    assert np.array_equal(got[0][:4], pos) and not np.any(got[0][4:])
    assert got[1:] == (np.float32(scan[0]), np.float32(scan[1]), scan[2])
    for bad in (dict(n_grid=7), dict(n_grid=513), dict(az_min=1.0, az_max=1.0), dict(az_min=0.0, az_max=6.3),
                dict(az_min=float("nan")), dict(az_max=float("inf"))):
        kw = dict(az_min=scan[0], az_max=scan[1], n_grid=scan[2])
        kw.update(bad)
        with pytest.raises(dnrp.DnrpError) as e:
            phy.set_rx_aoa(pos, **kw)
        assert e.value.code == EINVAL
        assert phy.rx_aoa_cfg()[1:] == got[1:]  # a refused call changes nothing
    cfg = dnrp._aoa_cfg(pos, *scan)
    cfg.reserved = 1
    assert dnrp.lib().dnrp_ctx_set_rx_aoa(phy._ctx, dnrp.C.byref(cfg)) == EINVAL
    phy.set_rx_aoa(None)
    assert phy.rx_aoa_cfg() is None
    phy.close()
    one = _phy((1, 1, 1, 2, 1, 1))
    with pytest.raises(dnrp.DnrpError) as e:
        one.set_rx_aoa(AC.ula(1))
    assert e.value.code == EINVAL and one.rx_aoa_cfg() is None
    one.set_rx_aoa(None)  # off is always accepted
    one.close()


def test_new_setting_holds_from_the_next_call(monkeypatch):
    import dnrp
    name = "ula4_td"
    g, ws = AC.geometry(name), AC.windows(name)
    _clean_env(monkeypatch)
    phy = _context(g)
    scan_a, scan_b = g["scan"], (g["scan"][0], g["scan"][1], 91)
    phy.set_rx_aoa(g["pos"], *scan_a)
    ps = dnrp.psdef(*g["psd"])
    n, S = len(ws), g["S"]
    dev = torch.device("cuda:0")
    iq = torch.from_numpy(np.stack([w["win"] for w in ws]).view(np.float32).reshape(n, g["n_rx"], S, 2)).to(dev)
    pcc_llr = torch.zeros((n, 196), dtype=torch.int16, device=dev)
    pdc_llr = torch.zeros((len(g["req"]), g["sz"]["G"]), dtype=torch.int16, device=dev)
    reqs = [dnrp.PdcReq(ps, i, ws[i]["nid"], ws[i]["pt"]) for i in g["req"]]
    phy.rx_pcc_batch(_reports(g, ws), iq, pcc_llr)
    phy.rx_pdc_batch(reqs, iq, pdc_llr)
    phy.set_rx_aoa(g["pos"], *scan_b)  # the call above may still be in flight: it keeps the setting it read
    assert phy.rx_pdc_batch([], iq, pdc_llr) is None  # an empty batch: DNRP_OK, nothing launched, the rows stay
    phy.sync()
    first = phy.rx_aoa(len(reqs))
    phy.rx_pdc_batch(reqs, iq, pdc_llr)
    phy.sync()
    second = phy.rx_aoa(len(reqs))
    phy.close()
    assert np.array_equal(first["R"], second["R"])
    for rows, scan in ((first, scan_a), (second, scan_b)):
        for r in range(len(reqs)):
            ref = AC.estimate(g["pos"], *scan, rows["R"][r], g["n_rx"])
            assert rows["grid_idx"][r] == ref["grid_idx"] and abs(float(rows["az_rad"][r]) - ref["az_rad"]) <= 1e-6
    assert first["grid_idx"][0] > scan_b[2]  # 65 deg: index 155 of 181, 77 or 78 of 91
