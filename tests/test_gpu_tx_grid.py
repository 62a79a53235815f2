"""GPU TX parity on the kernel forms of launch_tx that no other TX test reaches (tests/tx_grid_cases.py;
tests/test_tx_grid_host.py proves the coverage), under the gates of test_tx_parity (_check_tx, unchanged:
relative L2 <= 1e-4 per antenna against the oracle, GI and tail exactly zero, every sample written over the
poison). Each run asserts through the read-back dnrp_tx_last_form that the form it is there for ran, and that
the read-back equals the host-only twin dnrp_tx_form_for that the host file counts with.

 - tx_kernel_wave<10, 9, 22> by each cause that keeps a 1024-point 10/9 packet off the streaming kernel:
   a 7-pattern STF (u = 1), an output pointer 8 bytes past a 16-byte boundary, 8 spatial streams at 64-QAM;
 - tx_kernel_wave<10, 9, 4> (os_min 2) and <0, 0, 0> (40/27);
 - PDC bytes read in place (more than 8192 bytes per symbol run), wave and block kernel;
 - the streaming kernel's modes TXS_TXDIV and TXS_SM (a codebook whose W is no permutation), TXS_SISO with
   N_TX > 1 (TM3 / TM7 beamforming), 8 spatial streams with a 4 KiB byte window, each with and without the
   256-QAM form where the mode has both, the 256-QAM ones also on the matrix cores (DNRP_TX_MFMA = 1, 2);
 - the windowed instantiation (dnrp_ctx_set_tx_windowing(0.25)) of the wave classes and of every streaming
   mode that tests/test_gpu_tx_window.py does not reach, against that file's numpy reference.
"""
import numpy as np
import pytest

import test_gpu_parity as P
import test_gpu_tx_window as W
import tx_grid_cases as G

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _check_form(name, phy, windowed, mfma=0):
    form = phy.tx_last_form()
    want = dict(G.CASES[name][4], windowed=int(windowed))
    if form["family"] == "stream":
        want["mfma"] = mfma
    for k, v in want.items():
        assert form[k] == v, (name, k, form)
    assert form == G.host_form(name, windowed), (name, form, G.host_form(name, windowed))
    print("tx grid", name, form)


def _parity(name, monkeypatch, mfma=0):
    monkeypatch.setitem(P.TX_CASES, name, G.spec5(name))
    phy = P._tx_parity(name, misalign=G.CASES[name][3])
    _check_form(name, phy, False, mfma)
    phy.close()


@pytest.mark.parametrize("name", G.NAMES)
def test_tx_grid_parity(name, monkeypatch):
    monkeypatch.delenv("DNRP_TX_MFMA", raising=False)
    _parity(name, monkeypatch)


@pytest.mark.parametrize("name", G.MFMA)
@pytest.mark.parametrize("form", [1, 2])
def test_tx_grid_matrix_blocks(name, form, monkeypatch):
    monkeypatch.setenv("DNRP_TX_MFMA", str(form))
    _parity(name, monkeypatch, mfma=form)


@pytest.mark.parametrize("name", G.WINDOWED)
def test_tx_grid_windowed(name, monkeypatch):
    """the numpy reference without windowing reproduces the oracle at the case's own ratio (1e-6); with it, the
    GPU's windowed form is within 1e-4 per antenna"""
    import dnrp
    import oracle_py as O
    monkeypatch.delenv("DNRP_TX_MFMA", raising=False)
    psd, ctx, cb, misalign, _ = G.CASES[name]
    pcc, pdc, descs, g = G.windowed_packets(name)
    ocf = O.cfg(ctx[0], ctx[1], ctx[3], ctx[4], ctx[5])
    for i, (d, got) in enumerate(zip(descs, G.windowed_reference(name, None))):
        ref, _ = O.tx(ocf, O.psdef(*psd), pcc[i], pdc[i], g["S"], codebook=cb, network_id=d.network_id,
                      plcf_type=d.plcf_type, phase=float(np.float32(d.iq_phase_rad)),
                      phase_inc=float(np.float32(d.iq_phase_increment_s2s_post_resampling_rad)))
        for a in range(ref.shape[0]):
            nr = np.linalg.norm(ref[a])
            assert np.linalg.norm(got[a] - ref[a]) <= 1e-6 * (nr if nr > 0 else 1.0), (name, i, a)
    phy = dnrp.Phy(*ctx, max_batch=4)
    for nid in range(100, 104):
        phy.add_network_id(nid)
    phy.set_tx_windowing(G.FRACTION)
    iq = P._gpu_tx(phy, dnrp.psdef(*psd), descs, pcc, pdc, g["S"], misalign)
    _check_form(name, phy, True)
    phy.close()
    for i, ref in enumerate(G.windowed_reference(name, G.FRACTION)):
        W.check_tx(iq[i], ref, g["keep"], (name, G.FRACTION, i))


def test_tx_last_form_before_the_first_batch():
    import dnrp
    phy = dnrp.Phy(1, 1, 1, max_batch=1)
    with pytest.raises(dnrp.DnrpError) as e:
        phy.tx_last_form()
    assert e.value.code == -7  # DNRP_ESTATE
    phy.close()
