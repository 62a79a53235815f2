"""The MIMO report options on the GPU (dnrp_ctx_set_rx_mimo_report, dnrp_rx_mimo_detail; kernels/rx_mimo.hip
rx_mimo_detail_kernel). Inputs and the numpy model: tests/mimo_report_cases.py, its proof against hand-computed
examples and the conditions on the seeds: tests/test_rx_mimo_report_host.py.

1. Default (0, 0, 0); a context toggled to (2, 1, 1) and back is a never-toggled one, report for report; the new
   kernel did not run and dnrp_rx_mimo_detail returns DNRP_ESTATE.
2. (0, 0, 1): the reference's default through the new kernel, indices against the oracle's.
3. Every metric x search start: the scores against the model fed the device's own stage, the indices the first
   best of the device's own scores and the model's pick where its margin exceeds the tolerance.
4. The rank / precoder report: noise floor, rates against the model, the selection implied by the device's own
   rates, rank-one and unitary channels.
5. The same window through the plain Y path, the epoch receiver and the fused receiver (its zd stage).
6. Plumbing: rows without reports, request order, refused arguments, a spatial-multiplexing packet.

SCORE_DIFF / RATE_DIFF: the largest |device - model| measured on MI355X per geometry, in units of the packet's
largest score / rate; the bound is ten times that (float sums in another order than numpy's, hypotf, log2f) and
never looser than the caps 1e-4 (scores) and 1e-3 (rates) of mimo_report_cases.
"""
import numpy as np
import pytest

import mimo_report_cases as MR
import oracle_py as O
import phy_fixtures as F
import rx_grid_cases as RG
import rx_run_helpers as H
from rx_run_helpers import clean_env as _clean_env

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -7
# measured on the first MI355X run (geometry: value); see the module docstring
# scores: the largest over the six settings; rates: over the batch and, for t2r2 / t4r4, the rank-one windows (their
# G is near singular in the second direction: 1.806e-06 / 1.173e-05; the batches alone 1.115e-07 / 6.799e-07) and the
# unitary windows (6.911e-08 / 8.647e-08)
SCORE_DIFF = {"t2r2": 5.633e-07, "t4r4": 1.847e-07, "t2r4": 1.822e-07, "t1r2": 1.572e-07, "t2r8": 1.552e-07}
RATE_DIFF = {"t2r2": 1.806e-06, "t4r4": 1.173e-05, "t2r4": 8.733e-08, "t1r2": 9.886e-08, "t2r8": 1.154e-07,
             "tm2_sm2": 1.032e-07}
# sinr_eff_dB = 10 log10(2^x - 1), x = rate[RI] / RI in [1, 14], in float against double: x carries half an ulp
# (6e-8 x ln2 2^x / (2^x - 1) 4.34 < 6e-6 dB), exp2f two (2.4e-7 relative, doubled by the subtraction at 2^x >= 2:
# 2e-6 dB), log10f two of at most 42 dB (1e-5 dB)
SINR_TOL_DB = 1.0e-4
SETTINGS = [(m, a) for m in (0, 1, 2) for a in (0, 1)]
# the stage of the epoch receiver and the fused receiver's zd stage against the Y path's, as measured: bit-identical
PATHS_H_IDENTICAL = {"epoch": True, "fused": True}


def _bound(measured, cap):
    return cap if measured is None else min(cap, 10.0 * measured)


def _phy(ctx, lr=1, max_batch=MR.N_PACKETS):
    return H.phy(ctx, lr, max_batch)


def _rx(phy, psd, windows, reports, reqs, want_report=True, detail=False):
    """rx_run_helpers.rx as (PDC LLRs (torch, host), PDC reports or None, detail rows or None)"""
    r = H.rx(phy, psd, windows, reports, reqs, pcc_report=False, pdc_report=want_report, detail=detail)
    return r.pdc_llr, r.rep2, r.rows


def _sync_reports(g, ws):
    import dnrp
    return [dnrp.SyncReport(w["off"], 0.0, 0.0, g["psd"][0], g["psd"][1], g["n_ts"]) for w in ws]


_same_reports = H.same_pdc_reports


def _run_windows(name, ws, setting, want_report=True, reqs=None, env_phy=None):
    g = MR.geometry(name)
    phy = env_phy or _phy(g["ctx"])
    phy.set_rx_mimo_report(*setting)
    reqs = reqs if reqs is not None else [(i, w["nid"], w["pt"]) for i, w in enumerate(ws)]
    out = _rx(phy, g["psd"], [w["win"] for w in ws], _sync_reports(g, ws), reqs, want_report, detail=bool(setting[2]))
    counts = {k: phy.kernel_time_total(k)[1] for k in ("rx_mimo_detail", "rx_fused", "rx_epoch", "rx_pdc")}
    if env_phy is None:
        phy.close()
    return g, out, counts


_DEV = {}


def _batch(name, metric, all_w, monkeypatch):
    """the geometry's batch of 8 under (metric, all_w, 1), run once: (geometry, reports, rows)"""
    key = (name, metric, all_w)
    if key not in _DEV:
        _clean_env(monkeypatch)
        g, (_, rep, rows), counts = _run_windows(name, MR.batch(name), (metric, all_w, 1))
        assert counts["rx_mimo_detail"] == 1, counts
        _DEV[key] = (g, rep, rows)
    return _DEV[key]


def _stage(g, row):
    assert (int(row["N_RX"]), int(row["N_TS"])) == (g["n_rx"], g["n_ts"])
    H = row["H"]
    assert not np.any(H[g["n_rx"]:]) and not np.any(H[:, g["n_ts"]:])  # zero beyond N_RX / N_TS
    return H[:g["n_rx"], :g["n_ts"], :].astype(np.complex128)


# ---------------------------------------------------------------- 1. default and toggle
@pytest.mark.parametrize("name", ["t2r2", "t4r4"])
def test_default_and_toggle(name, monkeypatch):
    import dnrp
    _clean_env(monkeypatch)
    g, ws = MR.geometry(name), MR.batch(name)
    fresh = _phy(g["ctx"])
    assert fresh.rx_mimo_report() == (0, 0, 0)
    with pytest.raises(dnrp.DnrpError) as e:
        fresh.rx_mimo_detail(1)  # before any PDC call
    assert e.value.code == ESTATE
    _, (llr_a, rep_a, _), counts = _run_windows(name, ws, (0, 0, 0), env_phy=fresh)
    assert counts["rx_mimo_detail"] == 0, counts
    fresh.close()

    phy = _phy(g["ctx"])
    phy.set_rx_mimo_report(2, 1, 1)
    assert phy.rx_mimo_report() == (2, 1, 1)
    _, (llr_b, rep_b, _), counts = _run_windows(name, ws, (0, 0, 0), env_phy=phy)
    assert phy.rx_mimo_report() == (0, 0, 0)
    assert counts["rx_mimo_detail"] == 0, counts
    assert torch.equal(llr_a, llr_b)
    _same_reports(rep_a, rep_b)
    with pytest.raises(dnrp.DnrpError) as e:
        phy.rx_mimo_detail(1)  # the PDC call ran with detail = 0
    assert e.value.code == ESTATE
    phy.close()


# ---------------------------------------------------------------- 2. the reference's default through the new kernel
def _against_oracle(tag, ocf, ops, w, fp, cfo, nid, pt, rep, row):
    ref = O.rx(ocf, ops, w, fp, cfo, nid, pt)
    want = [0xFFFFFFFF if o == O.MIMO_REF_UNDEFINED else o for o in (ref["mimo_idx"], ref["mimo_idx_reciprocal"])]
    assert [int(row["idx_tx"]), int(row["idx_rx"])] == want, (tag, row["idx_tx"], row["idx_rx"], want)
    assert (rep.mimo_N_TS_other, rep.tm_3_7_beamforming_idx, rep.tm_3_7_beamforming_reciprocal_idx) == \
        (ref["mimo_N_TS_other"], want[0], want[1]), tag


@pytest.mark.parametrize("name", MR.BATCH_GEOMETRIES)
def test_reference_default_through_the_new_kernel(name, monkeypatch):
    g, rep, rows = _batch(name, 0, 0, monkeypatch)
    for r, w in enumerate(MR.batch(name)):
        _against_oracle((name, r), g["ocf"], g["ops"], w["win"], w["off"], 0.0, w["nid"], w["pt"], rep[r], rows[r])


def test_reference_default_at_10_9(monkeypatch):
    _clean_env(monkeypatch)
    psd, ctx, lr, snrs, cb = F.PARITY_CASES["tm5_u2b4"]
    u_max, b_max, n_rx, os_min, L, M = ctx
    ops, ocf = O.psdef(*psd), O.cfg(u_max, b_max, os_min, L, M, lr=lr)
    w, reports, nids, types, _, _ = RG.rx_windows(np.random.default_rng(11), ops, ocf, n_rx, (max(snrs),), cb)
    phy = _phy(ctx, lr)
    phy.set_rx_mimo_report(0, 0, 1)
    _, rep, rows = _rx(phy, psd, w[:1], reports[:1], [(0, nids[0], types[0])], detail=True)
    assert phy.kernel_time_total("rx_mimo_detail")[1] == 1
    phy.close()
    _against_oracle("tm5_u2b4", ocf, ops, w[0], reports[0].fine_peak_time, float(np.float32(reports[0].cfo_fractional_rad)),
                    nids[0], types[0], rep[0], rows[0])


# ---------------------------------------------------------------- 3. scores
@pytest.mark.parametrize("name", MR.BATCH_GEOMETRIES)
@pytest.mark.parametrize("metric,all_w", SETTINGS)
def test_scores(name, metric, all_w, monkeypatch):
    g, rep, rows = _batch(name, metric, all_w, monkeypatch)
    tol = _bound(SCORE_DIFF[name], MR.SCORE_CAP)
    worst, decisions, left_out = 0.0, 0, 0
    for r in range(MR.N_PACKETS):
        H = _stage(g, rows[r])
        model = {sd: MR.search(H, sd, metric, all_w) for sd in ("tx", "rx")}
        fin = [np.abs(m[1][np.isfinite(m[1])]) for m in model.values()]
        scale = max((float(v.max()) for v in fin if len(v)), default=1.0) or 1.0
        for sd, n_virt in (("tx", g["n_ts"]), ("rx", g["n_rx"])):
            idx_m, sc_m, margin = model[sd]
            sc_d, idx_d = rows[r]["score_" + sd], int(rows[r]["idx_" + sd])
            assert np.array_equal(np.isnan(sc_d), np.isnan(sc_m)), (name, r, sd)
            if np.isfinite(sc_m).any():
                worst = max(worst, float(np.nanmax(np.abs(sc_d.astype(np.float64) - sc_m))) / scale)
            assert idx_d == (0 if n_virt == 1 else MR.first_best(sc_d, metric)), (name, r, sd, idx_d)
            if n_virt in (2, 4):
                decisions += 1
                if margin / scale > tol:
                    assert idx_d == idx_m, (name, r, sd, idx_d, idx_m, margin / scale)
                else:
                    left_out += 1
            else:
                assert idx_d == idx_m, (name, r, sd)
        assert (rep[r].tm_3_7_beamforming_idx, rep[r].tm_3_7_beamforming_reciprocal_idx, rep[r].mimo_N_TS_other) == \
            (int(rows[r]["idx_tx"]), int(rows[r]["idx_rx"]), g["n_ts"]), (name, r)
    print(f"mimo scores {name} metric {metric} all_w {all_w}: device - model {worst:.3e} of the largest score, "
          f"bound {tol:.3e}; {left_out} of {decisions} decisions inside the tolerance")
    assert worst <= tol, (name, metric, all_w, worst)
    assert decisions and left_out <= 0.10 * decisions, (name, left_out, decisions)


def test_options_change_the_picks(monkeypatch):
    """on the device's own results: within a batch the metrics and the search starts pick apart"""
    for name in ("t2r2", "t4r4"):
        col = {s: [(int(x["idx_tx"]), int(x["idx_rx"])) for x in _batch(name, s[0], s[1], monkeypatch)[2]] for s in SETTINGS}
        assert col[(0, 0)] != col[(1, 0)] and col[(0, 0)] != col[(2, 0)] and col[(1, 0)] != col[(2, 0)], name
        for m in (0, 1, 2):
            assert col[(m, 0)] != col[(m, 1)], (name, m)


# ---------------------------------------------------------------- 4. rank report
def _check_rank_rows(name, g, rows, tol):
    """the checks of one set of rows; returns (worst rate deviation, decisions, left out)"""
    worst, decisions, left_out = 0.0, 0, 0
    for r in range(len(rows)):
        row = rows[r]
        H = _stage(g, row)
        nv, nvu = float(row["nv"]), float(row["nv_used"])
        assert nv > 0.0 and abs(nvu - MR.nv_used(nv, H, g["n_rx"], g["n_ts"])) <= 1e-6 * nvu, (name, r, nv, nvu)
        rc_d = row["rate_cb"]
        rc_m = MR.rates(H, nvu)
        assert np.array_equal(np.isnan(rc_d), np.isnan(rc_m)), (name, r)
        scale = float(np.nanmax(rc_m))
        worst = max(worst, float(np.nanmax(np.abs(rc_d.astype(np.float64) - rc_m))) / scale)
        # the selection the device's own rates imply, exactly
        pmi, rate, RI, PMI, sinr, _ = MR.report(rc_d)
        assert [int(x) for x in row["pmi"]] == pmi and (int(row["RI"]), int(row["PMI"])) == (RI, PMI), (name, r)
        assert np.array_equal(row["rate"], np.array(rate, np.float32), equal_nan=True), (name, r)
        assert rate[RI.bit_length() - 1] / RI >= 1.0  # SINR_TOL_DB's condition
        assert abs(float(row["sinr_eff_dB"]) - sinr) <= SINR_TOL_DB, (name, r, row["sinr_eff_dB"], sinr)
        # the model's, where its margins allow
        pmi_m, _, RI_m, _, _, margins = MR.report(rc_m)
        for s in range(3):
            if np.isfinite(margins[s]):
                decisions += 1
                if margins[s] / scale > tol:
                    assert pmi[s] == pmi_m[s], (name, r, s, pmi[s], pmi_m[s])
                else:
                    left_out += 1
        if np.isfinite(margins[3]):
            decisions += 1
            if margins[3] / scale > tol:
                assert RI == RI_m, (name, r, RI, RI_m)
            else:
                left_out += 1
    return worst, decisions, left_out


@pytest.mark.parametrize("name", MR.BATCH_GEOMETRIES)
def test_rank_report(name, monkeypatch):
    g, _, rows = _batch(name, 0, 0, monkeypatch)
    tol = _bound(RATE_DIFF[name], MR.RATE_CAP)
    worst, decisions, left_out = _check_rank_rows(name, g, rows, tol)
    print(f"mimo rates {name}: device - model {worst:.3e} of the largest rate, bound {tol:.3e}; "
          f"{left_out} of {decisions} decisions inside the tolerance")
    assert worst <= tol, (name, worst)
    assert left_out <= 0.10 * max(1, decisions), (name, left_out, decisions)
    avail = [R <= min(g["n_ts"], g["n_rx"]) for R in (1, 2, 4)]
    for row in rows:
        assert [int(p) != MR.NONE for p in row["pmi"]] == avail, name


@pytest.mark.parametrize("name,cb", [("t2r2", 3), ("t4r4", 17)])
def test_rank_one_channel(name, cb, monkeypatch):
    _clean_env(monkeypatch)
    g, (_, rep, rows), _ = _run_windows(name, [MR.window(name, ("rank_one", cb, 1), seed=1)], (0, 0, 1))
    worst, _, _ = _check_rank_rows(name, g, rows, _bound(RATE_DIFF[name], MR.RATE_CAP))
    print(f"mimo rates {name} rank one: device - model {worst:.3e} of the largest rate")
    assert worst <= _bound(RATE_DIFF[name], MR.RATE_CAP)
    assert int(rows[0]["RI"]) == 1 and int(rows[0]["pmi"][0]) == cb == int(rows[0]["PMI"]), rows[0]
    assert int(rows[0]["idx_tx"]) == cb == rep[0].tm_3_7_beamforming_idx


@pytest.mark.parametrize("name", ["t2r2", "t4r4"])
def test_unitary_channel(name, monkeypatch):
    _clean_env(monkeypatch)
    g, (_, _, rows), _ = _run_windows(name, [MR.window(name, ("unitary",), seed=2)], (0, 0, 1))
    worst, _, _ = _check_rank_rows(name, g, rows, _bound(RATE_DIFF[name], MR.RATE_CAP))
    print(f"mimo rates {name} unitary: device - model {worst:.3e} of the largest rate")
    assert worst <= _bound(RATE_DIFF[name], MR.RATE_CAP)
    assert int(rows[0]["RI"]) == min(g["n_ts"], g["n_rx"]), rows[0]


# ---------------------------------------------------------------- 5. paths
def test_paths(monkeypatch):
    """Measured on MI355X: the epoch receiver's stage is bit-identical to the Y path's, and so is the fused
    receiver's zd stage (PATHS_H_IDENTICAL); the bound is one float ulp either way."""
    ws = [MR.window("C4", ("gauss", 0), seed=0)]
    out = {}
    for tag, env in (("ypath", {"DNRP_RX_EPOCH": "0"}), ("epoch", {"DNRP_RX_EPOCH": "2"}), ("fused", {"DNRP_RX_FUSED": "1"})):
        _clean_env(monkeypatch, **env)
        g, (_, rep, rows), counts = _run_windows("C4", ws, (1, 1, 1))
        out[tag] = (rows[0], counts)
        assert counts["rx_mimo_detail"] == 1, (tag, counts)
    assert out["ypath"][1]["rx_epoch"] == 0 and out["ypath"][1]["rx_fused"] == 0 and out["ypath"][1]["rx_pdc"] > 0, out["ypath"][1]
    assert out["epoch"][1]["rx_epoch"] > 0 and out["epoch"][1]["rx_fused"] == 0, out["epoch"][1]
    assert out["fused"][1]["rx_fused"] > 0, out["fused"][1]
    y = out["ypath"][0]
    for tag in ("epoch", "fused"):
        o = out[tag][0]
        a, b = y["H"].view(np.float32), o["H"].view(np.float32)
        ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
        same = np.array_equal(a, b)
        print(f"mimo stage {tag} against the Y path: {'bit-identical' if same else 'within %.2f ulp' % float(np.max(np.abs(a - b) / ulp))}")
        assert np.all(np.abs(a - b) <= ulp), tag
        assert same == PATHS_H_IDENTICAL[tag], tag
        assert (int(o["idx_tx"]), int(o["idx_rx"])) == (int(y["idx_tx"]), int(y["idx_rx"])), tag
        print(f"mimo nv {tag} against the Y path: {float(o['nv']):.9e} / {float(y['nv']):.9e}")
        assert float(o["nv"]) > 0.0 and float(y["nv"]) > 0.0, tag


# ---------------------------------------------------------------- 6. plumbing
def test_rows_without_reports_and_request_order(monkeypatch):
    import dnrp
    _clean_env(monkeypatch)
    name = "t2r2"
    g, ws = MR.geometry(name), MR.batch(name)[:3]
    phy = _phy(g["ctx"])
    _, (_, rep, rows), counts = _run_windows(name, ws, (1, 0, 1), want_report=False, env_phy=phy)
    assert rep is None and counts["rx_mimo_detail"] == 1, counts
    assert all(int(x["N_TS"]) == 2 and np.isfinite(x["score_tx"][2:6]).all() for x in rows)
    # requests [2, 0]: row 0 is slot 2, row 1 slot 0
    reqs = [(2, ws[2]["nid"], ws[2]["pt"]), (0, ws[0]["nid"], ws[0]["pt"])]
    _, (_, rep2, rows2), _ = _run_windows(name, ws, (1, 0, 1), reqs=reqs, env_phy=phy)
    for row, slot in ((0, 2), (1, 0)):
        assert rows2[row].tobytes() == rows[slot].tobytes(), (row, slot)
        assert rep2[row].tm_3_7_beamforming_idx == int(rows[slot]["idx_tx"])
    assert rows[0].tobytes() != rows[2].tobytes()
    with pytest.raises(dnrp.DnrpError) as e:
        phy.rx_mimo_detail(3)  # above the latest call's m
    assert e.value.code == EINVAL
    assert len(phy.rx_mimo_detail(2)) == 2
    for bad in ((3, 0, 1), (1, 2, 1), (1, 0, 2)):
        with pytest.raises(dnrp.DnrpError) as e:
            phy.set_rx_mimo_report(*bad)
        assert e.value.code == EINVAL and phy.rx_mimo_report() == (1, 0, 1)  # a refused call changes nothing
    # (1, 0, 0) without reports: nothing to compute, and the rows of the call before are gone
    _, (_, rep3, _), counts = _run_windows(name, ws, (1, 0, 0), want_report=False, env_phy=phy)
    assert rep3 is None and counts["rx_mimo_detail"] == 0, counts
    with pytest.raises(dnrp.DnrpError) as e:
        phy.rx_mimo_detail(1)
    assert e.value.code == ESTATE
    phy.close()


def test_spatial_multiplexing_packet(monkeypatch):
    import dnrp
    _clean_env(monkeypatch)
    name = "tm2_sm2"
    g = MR.geometry(name)
    assert g["sz"]["N_SS"] == 2 and g["n_ts"] == 2
    phy = _phy(g["ctx"])
    phy.set_rx_mode(dnrp.Phy.RX_MODE_SM_MMSE)
    _, (_, rep, rows), counts = _run_windows(name, [MR.window(name, ("gauss", 4), seed=4)], (0, 0, 1), env_phy=phy)
    phy.close()
    assert counts["rx_mimo_detail"] == 1 and int(rows[0]["N_TS"]) == 2 and int(rows[0]["N_RX"]) == 2
    worst, _, _ = _check_rank_rows(name, g, rows, _bound(RATE_DIFF[name], MR.RATE_CAP))
    print(f"mimo rates {name}: device - model {worst:.3e} of the largest rate")
    assert worst <= _bound(RATE_DIFF[name], MR.RATE_CAP)
    assert int(rows[0]["RI"]) in (1, 2) and rep[0].mimo_N_TS_other == 2
