"""TX OFDM windowing on the GPU (dnrp_ctx_set_tx_windowing, the reference's PHY_TX_OFDM_WINDOWING:
tx.cpp:881-908, dft/windowing.cpp:34-56) in every TX path, against a reference built here:

  * the oracle's transmitter at the resampling ratio 1/1 gives the DECT-rate symbol stream
    (oracle_dsp.cpp:286-287),
  * window() restates the option's rules in numpy: a window of N = roundf(N_b_DFT_os / 8 * fraction)
    samples; every symbol l >= 1 gets cp_l[n] = cp_l[n] * rc[n] + body_{l-1}[n] * rc[N-1-n], body_{l-1}
    the first N samples behind the prefix of the symbol before it, the STF's ahead of its cover
    sequence (tx.cpp:226-234: the stash is taken inside run_ifft_cp_scale, the cover applied after),
  * resample() is a numpy polyphase resampler (resampler.cpp:330-454 closed form: the Kaiser taps of
    oracle_py.kaiser at the parameters of oracle_py.query_param, delay = (len - 1) / 2, output m reads
    t = delay + m M, p = t // L, ph = t % L) followed by the phase-continuous mixer (mixer.cpp:27-65).

The helper is pinned first: without windowing it must reproduce oracle_py.tx at the real ratio to
<= 1e-6 relative L2 (measured 3e-8 .. 5e-8). The gate is the TX parity gate of test_gpu_parity.py:
relative L2 <= 1e-4 per packet and antenna over the packet, GI and slot tail exactly zero, every
sample written (poisoned output)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import oracle_py as O
import phy_fixtures as F

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

_libm = C.CDLL("libm.so.6")
_libm.cosf.argtypes = _libm.sinf.argtypes = [C.c_float]
_libm.cosf.restype = _libm.sinf.restype = C.c_float

TM1 = ((2, 2, 1, 1, 1, 3), (2, 2, 2, 1, 10, 9))       # block path, two antennas, N_b_DFT_os = 128
TM1_1_1 = ((2, 2, 1, 1, 1, 3), (2, 2, 2, 1, 1, 1))
U1_64 = ((1, 1, 1, 1, 0, 1), (1, 1, 1, 1, 10, 9))     # N_b_DFT_os = 64, u = 1: 7 STF patterns, STF CP 3/4
CONFIG = {"tm1": TM1, "tm1_1_1": TM1_1_1, "u1_64": U1_64,
          **{k: F.case(k) for k in ("os2_u2b2_tm1", "lm40_27_b12", "C3", "C4", "lm1_1_u8b16", "u2_in_u8b16",
                                    "tm5_u2b4", "tm6_u8b16_64qam")}}


# ---------------------------------------------------------------- the reference, in numpy
def phasor_arg(rad):
    """mixer_t::set_phase / set_phase_increment keep a float phasor (mixer.cpp:27-39): its argument."""
    r = float(np.float32(rad))
    return math.atan2(float(_libm.sinf(r)), float(_libm.cosf(r)))


def rising_edge(N):
    """raised_cosine_window_rising_edge (raised_cosine.cpp:30-56) in float."""
    n, Nf, f = np.arange(N, dtype=np.float32), np.float32(N), np.float32
    A = np.cos(((n - Nf) / Nf * f(np.pi) * f(0.5)).astype(np.float64)).astype(np.float32)
    return A * A


def window_length(Nd, fraction):
    # roundf: halves away from zero; the products used here are never near a half
    return int(math.floor(float(np.float32(Nd // 8) * np.float32(fraction)) + 0.5))


def geometry(psd, cft):
    u_max, b_max, _, os_min, L, M = cft
    ops = O.psdef(*psd)
    sz = O.packet_sizes(ops)
    d = O.dims(O.cfg(u_max, b_max, os_min, L, M), ops)
    d1 = O.dims(O.cfg(u_max, b_max, os_min, 1, 1), ops)
    Nd = d["N_b_DFT_os"]
    return dict(sz=sz, Nd=Nd, CP=d["CP_os"], STF_CP=d["STF_CP_os"], N_DF=sz["N_DF_symb"],
                pattern_len=16 * psd[1] * Nd // sz["N_b_DFT"], total=d1["N_no_GI_os"], S1=d1["N_packet_os_rs"],
                keep=d["N_no_GI_os_rs"], S=d["N_packet_os_rs"], N_occ=sz["N_b_OCC"])


def window(x, g, fraction):
    """x complex64 [N_TX, total] DECT-rate stream -> windowed copy (float products, then the sum)."""
    N = window_length(g["Nd"], fraction)
    assert 2 <= N <= g["CP"]
    rc = rising_edge(N)
    rci = rc[::-1].copy()
    len0, lenD = g["STF_CP"] + g["Nd"], g["CP"] + g["Nd"]
    assert x.shape[1] == len0 + g["N_DF"] * lenD
    cover = O.cover_sequence()
    y = x.copy()
    for l in range(1, g["N_DF"] + 1):
        b = len0 + (l - 1) * lenD
        if l == 1:  # the STF ahead of its cover sequence: the pattern's sign undone
            i = g["STF_CP"] + np.arange(N)
            body = x[:, i] * cover[np.minimum(i // g["pattern_len"], 8)]
        else:
            body = x[:, b - lenD + g["CP"]: b - lenD + g["CP"] + N]
        y[:, b:b + N] = (x[:, b:b + N] * rc).astype(np.complex64) + (body * rci).astype(np.complex64)
    return y


@functools.lru_cache(maxsize=None)
def taps(L, M, os_min):
    q = lambda k: np.float32(O.query_param(f"resampler_param_t::{k}"))
    LM = np.float32(max(L, M))
    h = O.kaiser(q(f"f_pass_norm[0][{os_min}]") / LM, q(f"f_stop_norm[0][{os_min}]") / LM,
                 q("PASSBAND_RIPPLE_DONT_CARE"), q(f"f_stop_att_dB[0][{os_min}]"))
    delay = (len(h) - 1) // 2
    h = np.concatenate([h * np.float32(L), np.zeros(-len(h) % L, np.float32)])
    return h.astype(np.float64), delay, len(h) // L - 1


def resample(x, cft, g, phase, inc):
    """x complex [N_TX, total] at the DECT rate -> complex64 [N_TX, S] at the hw rate, mixed."""
    _, _, _, os_min, L, M = cft
    out = np.zeros((x.shape[0], g["S"]), np.complex128)
    keep, Nx = min(g["keep"], g["S"]), x.shape[1]
    m = np.arange(keep, dtype=np.int64)
    if L == 1 and M == 1:
        out[:, :keep] = x[:, :keep]
    else:
        h, delay, hl = taps(L, M, os_min)
        t = delay + m * M
        p, ph = t // L, t % L
        xd = x.astype(np.complex128)
        for d in range(hl + 1):
            j = p - d
            ok = (j >= 0) & (j < Nx)
            out[:, :keep] += np.where(ok, xd[:, np.clip(j, 0, Nx - 1)], 0) * h[ph + d * L]
    ph0, pinc = phasor_arg(phase), phasor_arg(inc)
    if ph0 != 0.0 or pinc != 0.0:
        out[:, :keep] *= np.exp(1j * (ph0 + m * pinc))
    return out.astype(np.complex64)


def packets(name, n):
    """n packets of a configuration: bits and descriptors; packet 2 on with a mixer phase and increment,
    another network ID and PLCF type."""
    import dnrp
    psd, cft = CONFIG[name]
    g = geometry(psd, cft)
    rng = np.random.default_rng(0x717D0 + n)
    pcc = np.stack([O.pack_bits(F.random_bits(rng, 196)) for _ in range(n)])
    pdc = np.stack([O.pack_bits(F.random_bits(rng, g["sz"]["G"])) for _ in range(n)])
    descs = [dnrp.TxDesc(0, 100, 1, 5, 1.0, 0.0, 0.0, 0)]
    for i in range(1, n):
        descs.append(dnrp.TxDesc(0, 100 + i, 2, 5, 1.0, 0.7 * i, 1.3 * 2 * np.pi / g["Nd"], 0))
    return pcc, pdc, descs


@functools.lru_cache(maxsize=None)
def dect_streams(name, n):
    """The packets' DECT-rate streams (oracle at the ratio 1/1, unmixed), computed once per configuration
    and read-only."""
    psd, cft = CONFIG[name]
    g = geometry(psd, cft)
    pcc, pdc, descs = packets(name, n)
    ocf1 = O.cfg(cft[0], cft[1], cft[3], 1, 1)
    xs = []
    for i, d in enumerate(descs):
        x, _ = O.tx(ocf1, O.psdef(*psd), pcc[i], pdc[i], g["S1"], network_id=d.network_id, plcf_type=d.plcf_type)
        x = x[:, :g["total"]].copy()
        x.setflags(write=False)
        xs.append(x)
    return xs


def reference(name, n, fraction):
    """hw-rate reference of the n packets at `fraction` (None: no windowing)."""
    psd, cft = CONFIG[name]
    g = geometry(psd, cft)
    _, _, descs = packets(name, n)
    return [resample(x if fraction is None else window(x, g, fraction), cft, g, d.iq_phase_rad,
                     d.iq_phase_increment_s2s_post_resampling_rad) for x, d in zip(dect_streams(name, n), descs)]


@functools.lru_cache(maxsize=None)
def helper_pinned(name, n):
    """Helper self-check: without windowing it reproduces oracle_py.tx at the configuration's own ratio."""
    psd, cft = CONFIG[name]
    g = geometry(psd, cft)
    pcc, pdc, descs = packets(name, n)
    ocf = O.cfg(cft[0], cft[1], cft[3], cft[4], cft[5])
    worst = 0.0
    for i, (d, got) in enumerate(zip(descs, reference(name, n, None))):
        ref, _ = O.tx(ocf, O.psdef(*psd), pcc[i], pdc[i], g["S"], network_id=d.network_id, plcf_type=d.plcf_type,
                      phase=float(np.float32(d.iq_phase_rad)),
                      phase_inc=float(np.float32(d.iq_phase_increment_s2s_post_resampling_rad)))
        for a in range(ref.shape[0]):
            e = np.linalg.norm(got[a] - ref[a]) / np.linalg.norm(ref[a])
            worst = max(worst, e)
            assert e <= 1e-6, (name, i, a, e)
    print(f"helper self-check {name}: worst relative L2 {worst:.2e}")
    return True


# ---------------------------------------------------------------- the GPU side
def ctx(name, max_batch=8):
    import dnrp
    psd, cft = CONFIG[name]
    phy = dnrp.Phy(*cft, max_batch=max_batch)
    for nid in range(100, 104):
        phy.add_network_id(nid)
    return phy, dnrp.psdef(*psd)


def gpu_tx(phy, ps, descs, pcc, pdc, S):
    dev = torch.device("cuda:0")
    sz = phy.packet_sizes(ps)
    out = torch.empty((len(descs), sz["N_TX"], S, 2), dtype=torch.float32, device=dev)
    out.fill_(7.0)  # poison: every sample must be written
    phy.tx_batch(ps, descs, torch.from_numpy(pcc).to(dev), torch.from_numpy(pdc).to(dev), out)
    phy.sync()
    return out.cpu().numpy().view(np.complex64)[..., 0]


def check_tx(iq, ref, keep, tag):
    for a in range(ref.shape[0]):
        e = np.linalg.norm(iq[a, :keep] - ref[a, :keep]) / np.linalg.norm(ref[a, :keep])
        print(f"{tag} antenna {a}: relative L2 {e:.2e}")
        assert e <= 1e-4, (tag, a, e)
        assert np.all(iq[a, keep:] == 0), (tag, a)


def parity(name, n, fraction, s_pad=0):
    """s_pad: output rows of S + s_pad samples (the slot tail grows by s_pad zeros)."""
    assert helper_pinned(name, n)
    psd, cft = CONFIG[name]
    g = geometry(psd, cft)
    pcc, pdc, descs = packets(name, n)
    phy, ps = ctx(name)
    phy.set_tx_windowing(fraction)
    iq = gpu_tx(phy, ps, descs, pcc, pdc, g["S"] + s_pad)
    phy.close()
    assert iq.shape[2] == g["S"] + s_pad
    for i, ref in enumerate(reference(name, n, fraction)):
        check_tx(iq[i], ref, g["keep"], (name, fraction, i))


@pytest.mark.parametrize("name", ["tm1", "tm1_1_1"])
@pytest.mark.parametrize("fraction", [0.25, 0.3, 1.0])
def test_block_path(name, fraction):
    """tx_kernel, two antennas, runs of K = 3 symbols: N = 4, 5 (odd) and 16 (the whole prefix)."""
    assert window_length(128, fraction) == {0.25: 4, 0.3: 5, 1.0: 16}[fraction]
    parity(name, 2, fraction)


def test_smallest_window_and_u1_stf():
    """N_b_DFT_os = 64 at 0.25: N = 2, the smallest legal window; a u = 1 STF (7 patterns, STF prefix
    3/4 N_b_DFT_os), whose body start lies in pattern 3."""
    g = geometry(*CONFIG["u1_64"])
    assert window_length(g["Nd"], 0.25) == 2 and g["STF_CP"] == 48 and g["STF_CP"] // g["pattern_len"] == 3
    parity("u1_64", 2, 0.25)


@pytest.mark.parametrize("name", ["os2_u2b2_tm1", "lm40_27_b12"])
def test_other_taps(name):
    """os_min = 2 (45 taps) and 40/27 (the generic resampler form)."""
    parity(name, 2, 0.25)


@pytest.mark.parametrize("name,n", [("C3", 2), ("lm1_1_u8b16", 2), ("C4", 1), ("tm6_u8b16_64qam", 1)])
def test_1024_point(name, n):
    """N_b_DFT_os = 1024: the streaming kernel's windowed form at 10/9 (C3 SISO, C4 the one-hot
    transmit-diversity form, tm6_u8b16_64qam spatial multiplexing with symbols straddling bytes; a few
    packets run in several segments per packet, each behind a history piece), the wave path (runs of
    K = 6) at 1/1."""
    parity(name, n, 0.25)


@pytest.mark.parametrize("fraction", [0.02, 1.0])
def test_1024_point_window_edges(fraction):
    """The streaming kernel at N = 3 (odd, far below a wave's 64 lanes) and N = 128 = CP (both of a lane's
    prefix samples shaped)."""
    assert window_length(1024, fraction) == {0.02: 3, 1.0: 128}[fraction]
    parity("C3", 2, fraction)


def test_1024_point_wave_path_10_9():
    """An odd row length keeps 10/9 packets off the streaming kernel (its 16-B pair stores): tx_kernel_wave
    with the 10/9 polyphase blocks."""
    parity("C3", 2, 0.25, s_pad=1)


@pytest.mark.parametrize("name,n", [("C3", 2), ("C4", 1)])
@pytest.mark.parametrize("form", ["1", "2"])
def test_1024_point_matrix_blocks(name, n, form, monkeypatch):
    """DNRP_TX_MFMA = 1 / 2: the streaming kernel's matrix-core forms carry the same windowing."""
    monkeypatch.setenv("DNRP_TX_MFMA", form)
    parity(name, n, 0.25)


def test_scratch_path():
    """N_b_DFT_os = 4096: tx_big_window_kernel between tx_big_sym_kernel and tx_big_resample_kernel."""
    parity("u2_in_u8b16", 1, 0.25)


def test_scratch_path_two_passes(monkeypatch):
    """DNRP_TX_BIG_CAP=1: every packet in a scratch pass of its own, the window kernel launched per pass."""
    monkeypatch.setenv("DNRP_TX_BIG_CAP", "1")
    parity("u2_in_u8b16", 2, 0.25)


@pytest.mark.parametrize("name", ["tm1", "C3"])
def test_off_is_off(name):
    """Windowing set and reset to 0 leaves exactly the default transmitter (C3: the streaming kernel's
    default form again); turning it on changes the waveform."""
    psd, cft = CONFIG[name]
    g = geometry(psd, cft)
    pcc, pdc, descs = packets(name, 2)
    fresh, ps = ctx(name)
    want = gpu_tx(fresh, ps, descs, pcc, pdc, g["S"])
    fresh.close()
    phy, ps = ctx(name)
    phy.set_tx_windowing(0.25)
    on = gpu_tx(phy, ps, descs, pcc, pdc, g["S"])
    phy.set_tx_windowing(0)
    off = gpu_tx(phy, ps, descs, pcc, pdc, g["S"])
    phy.close()
    assert np.array_equal(off.view(np.uint32), want.view(np.uint32))
    for i in range(2):
        for a in range(want.shape[1]):
            e = np.linalg.norm(on[i, a] - want[i, a]) / np.linalg.norm(want[i, a])
            assert e > 1e-2, (name, i, a, e)


@pytest.mark.parametrize("name", ["tm1", "tm5_u2b4"])
@pytest.mark.parametrize("fraction", [0.25, 0.3, 1.0])
def test_loopback(name, fraction):
    """Windowed GPU TX through a fixed seeded mixing matrix, noiseless, into the GPU RX: every PCC and
    PDC LLR sign is the sent bit (the oracle's RX does the same on the numpy-windowed oracle TX)."""
    import dnrp
    psd, cft = CONFIG[name]
    g = geometry(psd, cft)
    sz, S, n_rx = g["sz"], g["S"], cft[2]
    pcc, pdc, _ = packets(name, 2)
    descs = [dnrp.TxDesc(0, 100 + i, 1 + i, 5, 1.0, 0.0, 0.0, 0) for i in range(2)]
    phy, ps = ctx(name)
    phy.set_tx_windowing(fraction)
    iq = gpu_tx(phy, ps, descs, pcc, pdc, S)
    H = F.mixing_matrix(np.random.default_rng(0x100B), n_rx, iq.shape[1])
    dev = torch.device("cuda:0")
    win = np.stack([F.channel(None, iq[i], n_rx, S, 0, 0.0, None, H=H) for i in range(2)])
    rx_in = torch.from_numpy(win.view(np.float32).reshape(2, n_rx, S, 2)).to(dev)
    pcc_llr = torch.zeros((2, 196), dtype=torch.int16, device=dev)
    pdc_llr = torch.zeros((2, sz["G"]), dtype=torch.int16, device=dev)
    reps = [dnrp.SyncReport(0, 0.0, 0.0, psd[0], psd[1], sz["N_eff_TX"]) for _ in range(2)]
    phy.rx_pcc_batch(reps, rx_in, pcc_llr)
    phy.rx_pdc_batch([dnrp.PdcReq(ps, i, 100 + i, 1 + i) for i in range(2)], rx_in, pdc_llr)
    phy.sync()
    phy.close()
    for i in range(2):
        assert np.array_equal(pcc_llr[i].cpu().numpy() > 0, np.unpackbits(pcc[i])[:196] == 1), (name, fraction, i)
        assert np.array_equal(pdc_llr[i].cpu().numpy() > 0, np.unpackbits(pdc[i])[:sz["G"]] == 1), (name, fraction, i)


def oob_share(x, g):
    """Out-of-band power share of a DECT-rate data field: Hann-windowed periodogram over 4 N_b_DFT_os
    samples hopped by N_b_DFT_os, power beyond |f| > N_b_OCC / 2 + 4 subcarriers over the total."""
    Nd = g["Nd"]
    df = x[g["STF_CP"] + Nd: g["total"]].astype(np.complex128)
    seg, w = 4 * Nd, np.hanning(4 * Nd)
    psd = np.zeros(seg)
    for s in range(0, len(df) - seg + 1, Nd):
        psd += np.abs(np.fft.fft(df[s:s + seg] * w)) ** 2
    f = np.abs(np.fft.fftfreq(seg, d=1.0 / seg)) / 4.0  # in subcarriers
    return psd[f > g["N_occ"] / 2 + 4].sum() / psd.sum()


def test_emissions():
    """lm1_1_u8b16 (the output is the DECT-rate stream): windowing at 0.25 lowers the data field's
    out-of-band power share (the reference arithmetic gives -6.2 dB)."""
    psd, cft = CONFIG["lm1_1_u8b16"]
    g = geometry(psd, cft)
    pcc, pdc, descs = packets("lm1_1_u8b16", 1)
    phy, ps = ctx("lm1_1_u8b16")
    plain = gpu_tx(phy, ps, descs, pcc, pdc, g["S"])[0, 0]
    phy.set_tx_windowing(0.25)
    shaped = gpu_tx(phy, ps, descs, pcc, pdc, g["S"])[0, 0]
    phy.close()
    a, b = oob_share(plain, g), oob_share(shaped, g)
    print(f"out-of-band share: plain {10 * np.log10(a):.2f} dB, windowed {10 * np.log10(b):.2f} dB, "
          f"change {10 * np.log10(b / a):.2f} dB")
    assert b < a


def test_window_too_short_is_refused():
    """A 64-point packet at fraction 0.1 (N = 1): DNRP_EINVAL, nothing launched."""
    import dnrp
    psd, cft = CONFIG["u1_64"]
    g = geometry(psd, cft)
    pcc, pdc, descs = packets("u1_64", 2)
    phy, ps = ctx("u1_64")
    phy.set_tx_windowing(0.1)
    dev = torch.device("cuda:0")
    out = torch.full((2, 1, g["S"], 2), 7.0, dtype=torch.float32, device=dev)
    with pytest.raises(dnrp.DnrpError) as e:
        phy.tx_batch(ps, descs, torch.from_numpy(pcc).to(dev), torch.from_numpy(pdc).to(dev), out)
    assert e.value.code == -1
    phy.sync()
    assert bool((out == 7.0).all())
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(dnrp.DnrpError) as e:
            phy.set_tx_windowing(bad)
        assert e.value.code == -1
    phy.close()
