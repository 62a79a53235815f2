"""GPU RX parity on the kernel instantiations the launchers choose from (N_RX, N_eff_TX, N_bps) that no other
parity table reaches (tests/rx_grid_cases.py; tests/test_rx_grid_host.py proves the coverage and the
inputs): every case against the oracle on identical windows under the gates of tests/test_gpu_parity.py
(_check_rx, unchanged: llr_gate, SNR reports within 0.05 dB, STO within 1e-3 samples, RMS within 1e-4
relative, MIMO report exact), and each run proves by launch counts (DNRP_TIMING=1) that the receiver it is
there for is the one that ran.

 - epoch receiver: all six (N_RX, N_eff_TX) pairs with the 256-QAM and the generic demapper, DNRP_RX_EPOCH=2
   below 4 RX antennas and unset with 4 (<4, 1, *>, <4, 2, *> and <4, 4, 0> are on the default path);
 - fused receiver (DNRP_RX_FUSED=1): all nine pairs, the 8-antenna ones at (2, 16, 8, 1, 10, 9) (76 800 bytes
   of LDS);
 - Y path (DNRP_RX_EPOCH=0): the rx_cells_kernel<R, T, false, NBPS> pairs, and the wave front end with 8
   antennas;
 - spatial multiplexing (SM_MMSE) with the checks of test_rx_sm_mmse_parity;
 - one class of each of epoch, fused and cells in chestim l mode, one with stride 3.
"""
import pytest

import oracle_py as O
import rx_grid_cases as G
from test_gpu_parity import _rx_parity, _rx_sm_parity

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

_ENV = ("DNRP_RX_EPOCH", "DNRP_RX_FUSED", "DNRP_RX_SNR_FRONT", "DNRP_RX_GROUP")


def _prepared(name, lr, stride):
    """the case's windows in the form _rx_parity takes, with a context of its own"""
    import dnrp
    psd, ctx, snrs, _ = G.CASES[name]
    u_max, b_max, n_rx, os_min, L, M = ctx
    phy = dnrp.Phy(u_max, b_max, n_rx, os_min, L, M, chestim_mode_lr=bool(lr), stride=stride, max_batch=4)
    for nid in range(100, 106):
        phy.add_network_id(nid)
    w, reports, nids, types, pdc, _ = G.windows(name)
    hard = [s >= 20.0 for s in snrs]
    return (phy, dnrp.psdef(*psd), O.psdef(*psd), w, reports, nids, types, pdc, hard,
            lambda i: G.oracle(name, i, lr, stride))


def _run(name, receiver, lr, stride, monkeypatch):
    import dnrp
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in G.env_of(name, receiver).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("DNRP_TIMING", "1")
    psd, ctx, _, _ = G.CASES[name]
    assert G.wave_geometry(psd, ctx) or receiver == "ypath", name
    if receiver == "fused":  # the launch's LDS, N_RX wave regions, fits one CU: a parity case
        assert int(dnrp.query_table("fused_lds_bytes", ctx[2])[0]) <= 160 * 1024
    phy = _rx_parity((name, receiver, lr, stride), stride, _prepared(name, lr, stride))
    n_epoch = phy.kernel_time_total("rx_epoch")[1]
    n_fused = phy.kernel_time_total("rx_fused")[1]
    n_cells = phy.kernel_time_total("rx_pdc")[1]
    phy.close()
    counts = (n_epoch, n_fused, n_cells)
    if receiver == "epoch":
        assert n_epoch > 0 and n_fused == 0, (name, counts)
    elif receiver == "fused":
        assert n_fused > 0 and n_epoch == 0, (name, counts)
    else:
        assert n_epoch == 0 and n_fused == 0 and n_cells > 0, (name, counts)


@pytest.mark.parametrize("name,receiver", [r for r in G.RUNS if r[1] != "sm"],
                         ids=[f"{n}-{r}" for n, r in G.RUNS if r != "sm"])
def test_rx_grid_parity(name, receiver, monkeypatch):
    _run(name, receiver, 1, 2, monkeypatch)


@pytest.mark.parametrize("name,receiver,lr,stride", G.VARIANTS,
                         ids=[f"{n}-{r}-{'lr' if lr else 'l'}-s{st}" for n, r, lr, st in G.VARIANTS])
def test_rx_grid_mode_and_stride(name, receiver, lr, stride, monkeypatch):
    _run(name, receiver, lr, stride, monkeypatch)


@pytest.mark.parametrize("name", [n for n, r in G.RUNS if r == "sm"])
def test_rx_grid_sm_mmse(name, monkeypatch):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DNRP_TIMING", "1")
    psd, ctx, snrs, _ = G.CASES[name]
    w, reports, nids, types, pdc, _ = G.windows(name)
    phy = _rx_sm_parity(name, psd, ctx, snrs, prepared=(w, reports, nids, types, pdc))
    counts = [phy.kernel_time_total(k)[1] for k in ("rx_epoch", "rx_fused", "rx_pdc")]
    phy.close()
    assert counts[0] == 0 and counts[1] == 0 and counts[2] > 0, (name, counts)  # the MMSE cells kernel
