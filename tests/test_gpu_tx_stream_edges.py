"""GPU TX parity at the edges of the streaming kernel's PDC byte staging and of its one-hot code table
(tests/tx_stream_edge_cases.py), under the gates of test_tx_parity (_check_tx, unchanged: relative L2 <= 1e-4
per antenna against the oracle, GI and tail exactly zero, every sample written over the poison). Each run
asserts through dnrp_tx_last_form that the streaming kernel ran in the form the case is there for, and that the
host-only twin dnrp_tx_form_for says the same.

 - every packet's ceil(G / 8) is no multiple of 16, so the last 16-byte chunk of its last symbol straddles the
   row's end; rows back to back (pdc_stride = ceil(G / 8)) and at a stride that is no multiple of 16 (unaligned
   d-bit loads); the last row ends with its allocation, ones behind every other row;
 - 256-QAM and 64-QAM through TXS_TXDIV1, BPSK (flipped points in slots of their own), four transmit streams,
   TXS_SM1 with a two-chunk window, TXS_SISO and TXS_TXDIV;
 - every packet has PCC and DRS cells in its first two DF symbols (asserted from "symbol_cells");
 - one segment per packet and two (the second starts with a history piece);
 - the windowed instantiation once.
The first output index of piece 0 (head of txs_emit) follows from the resampler class alone, and the streaming
family has one class (10/9 with 223 taps): its other parity cannot be reached through the library.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O
import test_gpu_parity as P
import test_gpu_tx_window as W
import tx_grid_cases as G
import tx_stream_edge_cases as E

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _phy(ctx):
    import dnrp
    phy = dnrp.Phy(*ctx, max_batch=4)
    for nid in range(100, 104):
        phy.add_network_id(nid)
    return phy


def _check_form(name, phy, ps, windowed):
    import dnrp
    psd, ctx, cb, _, want = E.CASES[name]
    form = phy.tx_last_form()
    for k, v in dict(want, family=G.STREAM, windowed=int(windowed), mfma=0).items():
        assert form[k] == v, (name, k, form)
    n = G.N_WINDOWED if windowed else E.N_ROWS
    twin = dnrp.tx_form_for(ctx, ps, [cb] * n, win_fraction=G.FRACTION if windowed else 0.0)
    assert form == twin, (name, form, twin)
    print("tx stream edge", name, form)


@pytest.mark.parametrize("name", E.NAMES)
def test_tx_stream_edge(name, monkeypatch):
    import dnrp
    monkeypatch.delenv("DNRP_TX_MFMA", raising=False)
    psd, ctx, cb, extra, _ = E.CASES[name]
    phy = _phy(ctx)
    ps = dnrp.psdef(*psd)
    sz = phy.packet_sizes(ps)
    S, nb = sz["N_samples_packet_os_rs"], (sz["G"] + 7) // 8
    assert nb % 16 != 0, (name, nb)  # the last chunk straddles the row's end
    pcc, pdc, flat, stride = E.rows(name, sz)
    assert stride == nb + extra and (extra == 0 or stride % 16 != 0), (name, stride)
    # PCC and DRS cells in the first DF symbols (pieces 2 and 3 of the kernel)
    cells = dnrp.query_table("symbol_cells", psd[1], sz["N_TS"], sz["N_eff_TX"], sz["N_DF_symb"]).reshape(-1, 3)
    assert cells[1:3, 0].sum() == 98 and cells[1:3, 2].sum() > 0, (name, cells[:3])
    descs = [dnrp.TxDesc(cb, 100 + i, 1 + i % 2, 5, 1.0, 0.4 * i, (0.9 * i) * 2 * np.pi / sz["N_b_DFT_os"], 0)
             for i in range(E.N_ROWS)]
    dev = torch.device("cuda:0")
    d_pdc = torch.from_numpy(flat).to(dev)
    assert d_pdc.numel() == (E.N_ROWS - 1) * stride + nb  # the last row ends with the allocation
    d_pcc = torch.from_numpy(pcc).to(dev)
    out = torch.full((E.N_ROWS, sz["N_TX"], S, 2), 7.0, dtype=torch.float32, device=dev)  # poison
    assert out.data_ptr() % 16 == 0
    arr = (dnrp.TxDesc * E.N_ROWS)(*descs)
    # dnrp_tx_batch itself: Phy.tx_batch takes the stride from a [n, stride] tensor, which the last row lacks
    rc = dnrp.lib().dnrp_tx_batch(phy._ctx, C.byref(ps), E.N_ROWS, arr, C.c_void_p(d_pcc.data_ptr()),
                                  C.c_void_p(d_pdc.data_ptr()), stride, C.c_void_p(out.data_ptr()), S, None)
    assert rc == 0, (name, rc)
    phy.sync()
    iq = out.cpu().numpy().view(np.complex64)[..., 0]
    _check_form(name, phy, ps, False)
    phy.close()
    ocf = O.cfg(ctx[0], ctx[1], ctx[3], ctx[4], ctx[5])
    for i, d in enumerate(descs):
        ref, n_tx = O.tx(ocf, O.psdef(*psd), pcc[i], pdc[i], S, codebook=cb, network_id=d.network_id,
                         plcf_type=d.plcf_type, gi=5, dac=float(np.float32(d.DAC_scale)),
                         phase=float(np.float32(d.iq_phase_rad)),
                         phase_inc=float(np.float32(d.iq_phase_increment_s2s_post_resampling_rad)))
        P._check_tx(iq[i], ref, sz, S, n_tx, (name, i))


def test_tx_stream_edge_windowed(monkeypatch):
    """the windowed instantiation of the one-hot form against the numpy reference of tests/test_gpu_tx_window.py
    (tests/test_gpu_tx_grid.py's recipe: packets, reference and gate)"""
    import dnrp
    monkeypatch.delenv("DNRP_TX_MFMA", raising=False)
    name = E.WINDOWED
    psd, ctx, cb, _, want = E.CASES[name]
    monkeypatch.setitem(G.CASES, name, (psd, ctx, cb, 0, want))
    pcc, pdc, descs, g = G.windowed_packets(name)
    phy = _phy(ctx)
    phy.set_tx_windowing(G.FRACTION)
    iq = P._gpu_tx(phy, dnrp.psdef(*psd), descs, pcc, pdc, g["S"], 0)
    _check_form(name, phy, dnrp.psdef(*psd), True)
    phy.close()
    for i, ref in enumerate(G.windowed_reference(name, G.FRACTION)):
        W.check_tx(iq[i], ref, g["keep"], (name, G.FRACTION, i))
