"""Cost of the angle-of-arrival report (dnrp_ctx_set_rx_aoa; not part of bench.py, where the
setting is off): rx_aoa_kernel's time per chunk of n C4 packets (mu = 8, beta = 16, TM5, N_RX = 4, 256-QAM, 1 slot,
L/M = 10/9) from the DNRP_TIMING=1 event timers, next to the launches it follows: the PDC phase's DRS pass
(rx_fft_pdc), the SNR chain (rx_pdc in the epoch path) and the epoch receiver.

One packet is transmitted on the GPU, turned into a plane wave on a 4-antenna half-wavelength line at --az degrees
and repeated into n windows. Prints one JSON line.
Usage: python tools/bench_aoa.py [--n 16384] [--n-grid 181] [--reps 5] [--az 33]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dect-nr-plus-sdr_amd"))
os.environ.setdefault("DNRP_TIMING", "1")

import torch  # noqa: E402

import dnrp  # noqa: E402

TIMERS = ("rx_aoa", "rx_fft_pdc", "rx_pdc", "rx_epoch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--n-grid", type=int, default=181)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--az", type=float, default=33.0)
    a = ap.parse_args()
    psd, (u_max, b_max, n_rx, os_min, L, M) = (8, 16, 1, 1, 5, 8), (8, 16, 4, 1, 10, 9)
    dev = torch.device("cuda:0")
    phy = dnrp.Phy(u_max, b_max, n_rx, os_min, L, M, max_batch=a.n)
    phy.add_network_id(100)
    ps = dnrp.psdef(*psd)
    sz = phy.packet_sizes(ps)
    S, G, n_tx = sz["N_samples_packet_os_rs"], sz["G"], sz["N_TX"]
    rng = np.random.default_rng(1)
    pcc = torch.from_numpy(rng.integers(0, 256, (1, 25), dtype=np.uint8)).to(dev)
    pdc = torch.from_numpy(rng.integers(0, 256, (1, (G + 7) // 8), dtype=np.uint8)).to(dev)
    x = torch.empty((1, n_tx, S, 2), dtype=torch.float32, device=dev)
    phy.tx_batch(ps, [dnrp.TxDesc(0, 100, 1, 5, 1.0, 0.0, 0.0, 0)], pcc, pdc, x)
    phy.sync()
    t = np.arange(n_tx)
    g = np.exp(2j * np.pi * (0.23 * t + 0.07 * t * t)) / np.sqrt(n_tx)
    pos = np.array([(0.0, 0.5 * r) for r in range(n_rx)], np.float32)
    steer = np.exp(2j * np.pi * pos[:, 1] * np.sin(np.deg2rad(a.az)))
    xc = torch.view_as_complex(x[0].contiguous()).to(torch.complex128)
    s = (torch.from_numpy(g).to(dev)[:, None] * xc).sum(0)
    win = torch.view_as_real((torch.from_numpy(steer).to(dev)[:, None] * s[None, :]).to(torch.complex64))
    rx_in = win[None].repeat(a.n, 1, 1, 1).contiguous()
    pcc_llr = torch.empty((a.n, 196), dtype=torch.int16, device=dev)
    pdc_llr = torch.empty((a.n, G), dtype=torch.int16, device=dev)
    reps = [dnrp.SyncReport(0, 0.0, 0.0, psd[0], psd[1], sz["N_eff_TX"]) for _ in range(a.n)]
    reqs = (dnrp.PdcReq * a.n)(*[dnrp.PdcReq(ps, i, 100, 1) for i in range(a.n)])
    phy.set_rx_aoa(pos, -np.pi / 2, np.pi / 2, a.n_grid)

    def chunk():
        phy.rx_pcc_batch(reps, rx_in, pcc_llr)
        phy.rx_pdc_batch(reqs, rx_in, pdc_llr)
        phy.sync()

    chunk()  # warm-up (tables, code objects)
    for nm in TIMERS:
        phy.kernel_time_total(nm)
    for _ in range(a.reps):
        chunk()
    kt = {nm: phy.kernel_time_total(nm) for nm in TIMERS}
    rows = phy.rx_aoa(a.n)
    err = np.abs(np.rad2deg(rows["az_rad"].astype(np.float64)) - a.az)
    # compulsory bytes: every DRS cell of the packet once per antenna, 8 B each (with four streams per DRS symbol
    # that is the symbols' whole rows)
    byts = a.n * n_rx * int(rows["n_cells"][0]) * 8
    ms = kt["rx_aoa"][0] / max(1, kt["rx_aoa"][1])
    print(json.dumps({
        "what": "rx_aoa_kernel per chunk of C4 packets, beside the launches of the PDC phase it follows",
        "n": a.n, "n_grid": a.n_grid, "reps": a.reps,
        "kernel_ms_per_chunk": {nm: round(v[0] / a.reps, 4) for nm, v in kt.items()},
        "launches_per_chunk": {nm: v[1] / a.reps for nm, v in kt.items()},
        "rx_aoa_drs_cell_bytes": byts, "rx_aoa_gb_per_s": round(byts / (ms * 1e-3) / 1e9, 1) if ms else None,
        "n_cells": int(rows["n_cells"][0]), "az_err_deg_max": float(err.max()),
        "rows_identical": bool((rows["R"] == rows["R"][0]).all())}))


if __name__ == "__main__":
    main()
