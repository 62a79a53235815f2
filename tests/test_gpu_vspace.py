"""Virtual space (dnrp_vspace_mix, kernels/vspace.hip) and channel scanner (dnrp_chscan_batch,
kernels/ring.hip) on the GPU against numpy restatements of vspace_t::wchannel_execute
(simulation/vspace.cpp:449-513), hw_simulator_t::clip_and_quantize (radio/hw_simulator.cpp:710-733) and
chscanner_t::scan (phy/rx/chscan/chscanner.cpp:38-141), fed with the library's own link realisations
(dnrp_channel_realization).

Noiseless sums within 2e-5 relative L2 per antenna (test_gpu_channel.py's bound for the same link
arithmetic); the split of a span over several calls and the ADC bit-exact; noise by the statistics
test_gpu_channel.py asks of dnrp_channel_batch; the scanner within 1e-4 (at most ~2e4 non-negative
float terms summed in >= 64 blocks: ~2e-5 on the energy, half that on the RMS); and the loop the mixer
closes: GPU TX -> virtual space in instalments -> continuous-stream sync -> ring gather -> GPU RX.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O
import phy_fixtures as F
from test_gpu_stream import _np_gather, _oracle_stream

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SENTINEL = 77.0
R1, STRIDE1, T1, N1 = 3001, 3008, 2 ** 40 + 17, 2600  # odd ring: 8-B stores; the span wraps the ring end


def _phy():
    import dnrp
    return dnrp.Phy(1, 2, 4, 1, 10, 9, max_batch=8)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.complex64)).view(np.float32).reshape(*a.shape, 2)).to("cuda:0")


def _cfg(kind, snr_db=None, seed=99):
    import dnrp
    # EVA profile at 800 ns rms and 7.68 MS/s: the largest tap delay is tens of samples (asserted below)
    return dnrp.ChannelCfg(kind, 1, 800.0, 900.0, 7680000, 0.7, dnrp.CH_NOISELESS_DB if snr_db is None else snr_db, 1.0,
                           seed)


def _emissions(own_gain=0.0, scale=1.0, shift=0):
    """seven emissions over three tx rows and three links, relative to the span start T1"""
    import dnrp
    rows = [  # t_start - T1, tx_row, length, link, own, gain
        (100, 0, 700, 0, 0, 0.9),     # overlaps the next for 300 samples
        (500, 1, 650, 3, 0, 0.5),
        (-300, 2, 700, 7, 0, 1.3),    # begins 300 samples before the span
        (2300, 0, 700, 3, 0, 0.7),    # runs past the span end; shares link 3
        (-2000, 1, 700, 0, 0, 1.1),   # entirely before the span
        (1300, 2, 600, 7, 0, 0.8),
        (1500, 1, 300, 0, 1, own_gain),  # own transmission over part of the one before
    ]
    return [dnrp.VspaceEmission(T1 + shift + t, row, ln, link, own, g * scale if not own else g, 0)
            for t, row, ln, link, own, g in rows]


def _tx(seed, n_rows=3, n_tx=2, S_tx=700):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_rows, n_tx, S_tx)) + 1j * rng.standard_normal((n_rows, n_tx, S_tx))).astype(np.complex64)


def _np_link(cfg, real, x, length, q, t, rx):
    """one emission through its N_TX links into antenna rx: q = t - t_start per sample (link.cpp:246-288)"""
    import dnrp
    out = np.zeros(len(t), np.complex128)
    for k in range(x.shape[0]):
        if cfg.kind == dnrp.CH_DOUBLY:
            for i, (d, a) in enumerate(zip(real["delay"][rx, k], real["amp"][rx, k])):
                qq = q - int(d)
                ok = (qq >= 0) & (qq < length)
                xv = np.where(ok, x[k, np.clip(qq, 0, length - 1)], 0)
                g = np.zeros(len(t), np.complex128)
                for P, ph in zip(real["period"][rx, k, i], real["phase_rev"][rx, k, i]):
                    g += np.exp(2j * np.pi * ((t % abs(int(P))) / float(P) + ph))
                out += float(a) * xv * g
        else:
            ok = (q >= 0) & (q < length)
            xv = np.where(ok, x[k, np.clip(q, 0, length - 1)], 0)
            out += xv * (real["coef"][rx, k] if cfg.kind == dnrp.CH_FLAT else 1.0)
    return out


def _np_vspace(cfg, ems, tx, n_rx, t_begin, n, only_own=False):
    """wchannel_execute without the noise, in double: foreign sum, detached while transmitting, own leakage"""
    import dnrp
    t = t_begin + np.arange(n, dtype=np.int64)
    real = {}
    s = np.zeros((n_rx, n), np.complex128)

    def add(e):
        if e.link not in real:
            real[e.link] = dnrp.channel_realization(cfg, e.link, tx.shape[1], n_rx)
        for r in range(n_rx):
            s[r] += float(np.float32(e.gain)) * float(np.float32(cfg.large_scale)) * _np_link(
                cfg, real[e.link], tx[e.tx_row], e.length, t - e.t_start, t, r)

    for e in ems:
        if not e.own and not only_own:
            add(e)
    for e in ems:
        if e.own:
            s[:, (t >= e.t_start) & (t < e.t_start + e.length)] = 0
    for e in ems:
        if e.own:
            add(e)
    return s


def _ring(n_ant, stride):
    return torch.full((n_ant, stride, 2), SENTINEL, dtype=torch.float32, device="cuda:0")


def _span(ring, ring_len, t_begin, n):
    """host complex copy of global samples [t_begin, t_begin + n) of every antenna"""
    z = ring.cpu().numpy().view(np.complex64)[..., 0]
    return z[:, (t_begin + np.arange(n)) % ring_len]


def _untouched(ring, ring_len, t_begin, n):
    z = ring.cpu().numpy()
    keep = np.ones(z.shape[1], bool)
    keep[(t_begin + np.arange(n)) % ring_len] = False
    return np.all(z[:, keep] == SENTINEL)


def _rel(got, ref):
    return np.linalg.norm(got - ref) / np.linalg.norm(ref)


def _case1(phy, kind, ems, tx, snr_db=None, adc=None, seed=99, t_begin=T1):
    cfg = _cfg(kind, snr_db, seed)
    ring = _ring(3, STRIDE1)
    phy.vspace_mix(cfg, ems, _dev(tx), ring, t_begin, N1, adc=adc, ring_len=R1)
    phy.sync()
    return cfg, ring


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_noiseless_parity(kind):
    import dnrp
    phy = _phy()
    assert T1 % R1 + N1 > R1  # the span holds the ring's wrap point
    ems, tx = _emissions(), _tx(70 + kind)
    cfg, ring = _case1(phy, kind, ems, tx)
    if kind == dnrp.CH_DOUBLY:
        assert dnrp.channel_realization(cfg, 0, 2, 3)["delay"].max() >= 5  # the delay line's tail is exercised
    got = _span(ring, R1, T1, N1)
    ref = _np_vspace(cfg, ems, tx, 3, T1, N1)
    for r in range(3):
        err = _rel(got[r], ref[r])
        print("noiseless", kind, r, err)
        assert err < 2e-5, (kind, r, err)
    assert np.all(got[:, 1500:1800] == 0)  # detached during the own transmission, no leakage at gain 0
    assert _untouched(ring, R1, T1, N1)


def test_many_emissions_in_one_tile():
    import dnrp
    phy = _phy()
    rng = np.random.default_rng(81)
    R, t_begin, n = 2048, 10 ** 6 + 3, 1500
    tx = _tx(82, n_rows=5, n_tx=1, S_tx=64)
    ems = [dnrp.VspaceEmission(t_begin + 600 + int(rng.integers(0, 256)), e % 5, 64, e % 4, 0, 0.3 + 0.05 * e, 0)
           for e in range(40)]
    cfg = _cfg(dnrp.CH_AWGN)
    ring = _ring(2, R)
    phy.vspace_mix(cfg, ems, _dev(tx), ring, t_begin, n)
    phy.sync()
    got = _span(ring, R, t_begin, n)
    ref = _np_vspace(cfg, ems, tx, 2, t_begin, n)
    for r in range(2):
        err = _rel(got[r], ref[r])
        print("many", r, err)
        assert err < 2e-5, (r, err)
    assert _untouched(ring, R, t_begin, n)


def test_own_leakage():
    import dnrp
    phy = _phy()
    ems, tx = _emissions(own_gain=0.05), _tx(83)
    cfg, ring = _case1(phy, dnrp.CH_FLAT, ems, tx)
    got = _span(ring, R1, T1, N1)
    ref = _np_vspace(cfg, ems, tx, 3, T1, N1)
    own = _np_vspace(cfg, ems, tx, 3, T1, N1, only_own=True)
    for r in range(3):
        err, err_own = _rel(got[r], ref[r]), _rel(got[r, 1500:1800], own[r, 1500:1800])
        print("leakage", r, err, err_own)
        assert err < 2e-5 and err_own < 2e-5, (r, err, err_own)  # inside the interval: the leaked signal alone
    assert np.abs(own[:, 1500:1800]).min() > 0


@pytest.mark.parametrize("kind", [0, 2])
def test_split_invariance_bit_exact(kind):
    phy = _phy()
    ems, tx = _emissions(own_gain=0.05), _tx(84)
    cfg, one = _case1(phy, kind, ems, tx, snr_db=20.0)
    parts = _ring(3, STRIDE1)
    tx_d = _dev(tx)
    for a, b in ((0, 1000), (1000, 1001), (1001, N1)):
        phy.vspace_mix(cfg, ems, tx_d, parts, T1 + a, b - a, ring_len=R1)
    phy.sync()
    assert torch.equal(one, parts)
    assert _untouched(parts, R1, T1, N1)
    if kind == 0:
        # the same span 2^32 samples later, emissions moved along: the same signal under other noise
        # (a 32-bit time counter in the noise key would repeat it)
        _, late = _case1(phy, kind, _emissions(own_gain=0.05, shift=2 ** 32), tx, snr_db=20.0, t_begin=T1 + 2 ** 32)
        d = _span(late, R1, T1 + 2 ** 32, N1) - _span(one, R1, T1, N1)
        n0 = 10 ** (-20.0 / 10)
        print("late", np.mean(np.abs(d) ** 2) / n0)
        assert np.mean(np.abs(d) ** 2) > n0  # two independent draws differ by 2 n0 on average
        assert np.mean(np.abs(d) ** 2) < 4 * n0  # and by the noise alone


def test_paired_stores():
    """an even ring, an even span start and aligned rows take the 16-B stores (the cases above, on an odd
    ring, the 8-B ones): the same parity and sentinel checks, an odd sample count (a lone last sample),
    and bit-equality with a split at odd samples, whose later parts store 8 B at a time"""
    phy = _phy()
    R, t0, n = 3000, T1 + 1, N1 - 1
    assert R % 2 == 0 and (t0 % R) % 2 == 0 and n % 2 == 1 and t0 % R + n > R and STRIDE1 % 2 == 0
    ems, tx = _emissions(own_gain=0.05, shift=1), _tx(87)
    tx_d = _dev(tx)
    cfg = _cfg(1)
    ring = _ring(3, STRIDE1)
    assert ring.data_ptr() % 16 == 0
    phy.vspace_mix(cfg, ems, tx_d, ring, t0, n, ring_len=R)
    phy.sync()
    got, ref = _span(ring, R, t0, n), _np_vspace(cfg, ems, tx, 3, t0, n)
    for r in range(3):
        err = _rel(got[r], ref[r])
        print("paired", r, err)
        assert err < 2e-5, (r, err)
    assert _untouched(ring, R, t0, n)
    cfg = _cfg(1, snr_db=20.0)
    one, parts = _ring(3, STRIDE1), _ring(3, STRIDE1)
    phy.vspace_mix(cfg, ems, tx_d, one, t0, n, ring_len=R)
    for a, b in ((0, 1024), (1024, 1501), (1501, 1502), (1502, n)):
        phy.vspace_mix(cfg, ems, tx_d, parts, t0 + a, b - a, ring_len=R)
    phy.sync()
    assert torch.equal(one, parts)
    assert _untouched(parts, R, t0, n)


def test_noise_statistics():
    import dnrp
    phy = _phy()
    n_rx, S = 4, 400000
    cfg = dnrp.ChannelCfg(dnrp.CH_AWGN, 0, 0.0, 0.0, 1, 1.0, 10.0, 0.8, 123)
    ring = _ring(n_rx, S)
    t_begin = 3 * S + 12345
    phy.vspace_mix(cfg, [], None, ring, t_begin, S)
    phy.sync()
    z = _span(ring, S, t_begin, S).astype(np.complex128)
    n0 = 10 ** ((-10 * np.log10(0.8) - 10.0) / 10)  # noise.cpp -> ch_awgn set_n0
    assert abs(np.mean(np.abs(z) ** 2) / n0 - 1) < 0.03
    assert abs(np.mean(z.real)) < 0.01 * np.sqrt(n0) and abs(np.mean(z.real * z.imag)) < 0.01 * n0
    for a in range(n_rx):
        for b in range(a + 1, n_rx):
            assert abs(np.mean(z[a] * np.conj(z[b]))) < 0.01 * n0, (a, b)  # antennas independent
        assert abs(np.mean(z[a, 1:] * np.conj(z[a, :-1]))) < 0.01 * n0, a  # white
    assert abs(np.mean(z[:, 1:] * np.conj(z[:, :-1]))) < 0.01 * n0


def _np_adc(x, clip, n_bits):
    """clip_re_im then quantize_re_im on float32 re / im, roundf exactly (half away from zero)"""
    lim = np.float32(clip)
    y = np.clip(x, -lim, lim).astype(np.float32)
    if n_bits:
        bw = np.float32(2) * lim / np.float32(2 ** n_bits)
        q = (y / bw).astype(np.float32)
        r = np.sign(q).astype(np.float64) * np.floor(np.abs(q.astype(np.float64)) + 0.5)
        y = (r.astype(np.float32) * bw).astype(np.float32)
    return y


def test_adc_bit_exact():
    import dnrp
    phy = _phy()
    ems, tx = _emissions(own_gain=0.05, scale=0.3), _tx(85)
    _, plain = _case1(phy, 1, ems, tx, snr_db=20.0, seed=5)
    x = plain.cpu().numpy()
    span = np.zeros(STRIDE1, bool)
    span[(T1 + np.arange(N1)) % R1] = True
    clipped = np.mean(np.abs(x[:, span]) > np.float32(0.6))
    print("clipped share", clipped)
    assert 0.005 < clipped < 0.2  # the clamp is at work, and not on everything
    for n_bits in (6, 0):
        _, ring = _case1(phy, 1, ems, tx, snr_db=20.0, seed=5, adc=dnrp.AdcCfg(0.6, n_bits))
        got = ring.cpu().numpy()
        want = x.copy()
        want[:, span] = _np_adc(x[:, span], 0.6, n_bits)
        assert np.array_equal(got, want), n_bits
    _, ring = _case1(phy, 1, ems, tx, snr_db=20.0, seed=5, adc=dnrp.AdcCfg(0.0, 6))  # no clip limit: unchanged
    assert torch.equal(ring, plain)


def test_argument_checks():
    import dnrp
    phy = _phy()
    L = dnrp.lib()
    tx = _dev(_tx(86))
    ring = _ring(3, STRIDE1)
    before = ring.clone()
    base = dict(ch=_cfg(1), adc=None, em=_emissions(), N_TX=2, tx=tx.data_ptr(), n_rows=3, S_tx=700, N_RX=3,
                ring=ring.data_ptr(), ring_len=R1, ant_stride=STRIDE1, t_begin=T1, n_samples=N1)

    def call(edit=None, **kw):
        a = dict(base, **kw)
        em = (dnrp.VspaceEmission * len(a["em"]))(*a["em"]) if a["em"] is not None else None
        if edit:
            edit(em)
        return L.dnrp_vspace_mix(phy._ctx, C.byref(a["ch"]) if a["ch"] is not None else None,
                                 C.byref(a["adc"]) if a["adc"] is not None else None, 7, em, a["N_TX"], a["tx"], a["n_rows"],
                                 a["S_tx"], a["N_RX"], a["ring"], a["ring_len"], a["ant_stride"], a["t_begin"], a["n_samples"],
                                 None)

    def em_field(i, name, value):
        def edit(em):
            setattr(em[i], name, value)
        return edit

    bad_kind, bad_pdp = _cfg(3), _cfg(2)
    bad_pdp.pdp_idx = 3
    bad = [dict(ch=None), dict(ring=None), dict(em=None), dict(tx=None), dict(N_TX=0), dict(N_TX=9), dict(N_RX=0),
           dict(N_RX=9), dict(ant_stride=R1 - 1), dict(n_samples=R1 + 1), dict(t_begin=-1), dict(S_tx=699), dict(n_rows=2),
           dict(adc=dnrp.AdcCfg(-0.5, 6)), dict(adc=dnrp.AdcCfg(0.6, 25)), dict(ch=bad_kind), dict(ch=bad_pdp)]
    for kw in bad:
        assert call(**kw) == -1, kw
    edits = [(4, "t_start", -1), (0, "length", 0), (0, "length", 701), (1, "tx_row", 3), (2, "gain", -0.1),
             (2, "gain", float("nan")), (2, "gain", float("inf")), (5, "reserved", 1)]
    for i, name, value in edits:
        assert call(em_field(i, name, value)) == -1, (i, name, value)
    assert call(n_samples=0) == 0
    phy.sync()
    assert torch.equal(ring, before)  # nothing ran: neither the refused calls nor the empty span
    assert call() == 0
    phy.sync()
    assert _untouched(ring, R1, T1, N1) and not torch.equal(ring, before)


def test_end_to_end_c2(monkeypatch):
    """two devices' packets from dnrp_tx_batch, mixed in two instalments into a ring the stream wraps,
    each instalment followed by the continuous-stream sync over the chunks it completed"""
    import dnrp
    monkeypatch.setenv("DNRP_TIMING", "1")
    rng = np.random.default_rng(91)
    name = "C2"
    psd, cfgt = F.CONFIGS[name]
    u_max, b_max, ntx, os_min, L, M = cfgt
    phy = dnrp.Phy(u_max, b_max, ntx, os_min, L, M, max_batch=64)
    for nid in (100, 101):
        phy.add_network_id(nid)
    ps = dnrp.psdef(*psd)
    sz = phy.packet_sizes(ps)
    S, G = sz["N_samples_packet_os_rs"], sz["G"]
    length = dnrp.tx_transmit_length(ps, 5, u_max, b_max, os_min, L, M)
    chunk, n_chunks, max_reports = 400, 24, 3  # test_sync_stream_c2's geometry
    sc = dnrp.SyncCfg(psd[0], psd[1], 1, chunk, max_reports)
    S_win = phy.sync_stream_window(sc)
    T = n_chunks * chunk + S_win
    R = T
    g0 = 5 * R + R // 3  # global time of stream sample 0: the ring wraps inside the stream
    times = [150, 1190, 2001, 3395, 5210, 6210, 7604, 8399]  # irregular, some next to chunk edges
    t_blank, own_at, own_len = 4300, 4280, 800  # a foreign packet wholly inside the receiver's own slot
    assert all(b - a >= length for a, b in zip(times, times[1:])) and own_at <= t_blank and t_blank + length <= own_at + own_len
    assert times[3] + length <= own_at and own_at + own_len <= times[4]
    n = len(times) + 1
    dev_of = [i % 2 for i in range(n)]  # device 0: network 100, PLCF type 1; device 1: network 101, type 2
    pcc = rng.integers(0, 256, (n, 25), dtype=np.uint8)
    pdc = rng.integers(0, 256, (n, (G + 7) // 8), dtype=np.uint8)
    descs = [dnrp.TxDesc(0, 100 + d, 1 + d, 5, 1.0, 0.0, 0.0, 0) for d in dev_of]
    tx = torch.empty((n, 1, S, 2), dtype=torch.float32, device="cuda:0")
    phy.tx_batch(ps, descs, torch.from_numpy(pcc).cuda(), torch.from_numpy(pdc).cuda(), tx)
    phy.sync()
    rms = float(np.sqrt(np.mean(np.abs(tx.cpu().numpy().view(np.complex64)[:, 0, :length, 0]) ** 2)))
    ems = [dnrp.VspaceEmission(g0 + t, i, length, 1 + dev_of[i], 0, 1.0 / rms, 0) for i, t in enumerate(times)]
    ems.append(dnrp.VspaceEmission(g0 + t_blank, n - 1, length, 1 + dev_of[n - 1], 0, 1.0 / rms, 0))
    assert own_len <= S
    ems.append(dnrp.VspaceEmission(g0 + own_at, 0, own_len, 0, 1, 0.0, 0))  # own slot, no leakage
    cfg = dnrp.ChannelCfg(dnrp.CH_AWGN, 0, 0.0, 0.0, 1, 1.0, 25.0, 1.0, 17)
    ring = torch.zeros((1, R, 2), dtype=torch.float32, device="cuda:0")
    state = phy.sync_stream_init(sc)
    half = n_chunks // 2
    cut = half * chunk + S_win  # the first instalment completes the windows of chunks 0..half-1
    got, chunk_of = [], []
    for part, (a, b) in enumerate(((0, cut), (cut, T))):
        phy.vspace_mix(cfg, ems, tx, ring, g0 + a, b - a)
        res, ck = phy.rx_sync_stream(sc, ring, g0 + part * half * chunk, half, state)
        got += list(res)
        chunk_of += [int(c) + part * half for c in ck]
    assert phy.kernel_time_total("vspace_mix")[1] > 0
    # occupancy as work_channel measures it: the detached slot holds noise alone, a packet's span does not
    parts, _ = phy.chscan(ring, [dnrp.ChscanReq(g0 + own_at + own_len - 1, own_len // 2, 2),
                                 dnrp.ChscanReq(g0 + times[0] + length - 1, length // 2, 2)])
    print("slot / packet rms", parts[0], parts[1])
    assert parts[0].max() < 0.5 * parts[1].min()
    assert phy.kernel_time_total("chscan")[1] > 0
    ring_h = ring.cpu().numpy().view(np.complex64)[..., 0]
    osc = O.sync_cfg(psd[0], psd[1], L=L, M=M, n_ant=1, chunk_len=chunk)
    ref, dup = _oracle_stream(osc, ring_h, g0, n_chunks, chunk, S_win, max_reports, state.sync_time_unique_limit)
    assert len(got) == len(ref), ([int(g["fine_peak_time"]) for g in got], [r[0] for r in ref])
    for g, k, (t, kr, r) in zip(got, chunk_of, ref):
        assert int(g["fine_peak_time"]) == t and k == kr
        assert int(g["N_eff_TX"]) == r["N_eff_TX"]
        assert abs(float(g["cfo_fractional_rad"]) - r["cfo_frac"]) < 2e-6
    assert int(state.not_unique) == dup
    # every packet on the air exactly once, next to its start; nothing from the detached slot
    fine = [int(g["fine_peak_time"]) - g0 for g in got]
    assert len(fine) == len(times), fine
    assert all(abs(f - t) <= state.sync_time_unique_limit for f, t in zip(fine, times)), fine
    assert not any(own_at - 64 <= f < own_at + own_len for f in fine), fine

    pre, S_in = 64, S + 256
    starts = [int(g["fine_peak_time"]) - pre for g in got]
    win_d = torch.zeros((len(got), 1, S_in, 2), dtype=torch.float32, device="cuda:0")
    phy.ring_gather(ring, starts, S_in, win_d)
    reps = dnrp.sync_reports(np.array(got, dtype=dnrp.SYNC_RESULT_DTYPE))
    reps["fine_peak_time"] = pre
    pcc_llr = torch.zeros((len(got), 196), dtype=torch.int16, device="cuda:0")
    pdc_llr = torch.zeros((len(got), G), dtype=torch.int16, device="cuda:0")
    phy.rx_pcc_batch(reps, win_d, pcc_llr)
    phy.rx_pdc_batch([dnrp.PdcReq(ps, i, 100 + dev_of[i], 1 + dev_of[i]) for i in range(len(got))], win_d, pdc_llr)
    phy.sync()
    hard = (pdc_llr.cpu().numpy() > 0).astype(np.uint8)
    for i in range(len(got)):
        assert np.array_equal(np.unpackbits(pdc[i])[:G], hard[i]), i


def _scan_ring():
    rng = np.random.default_rng(95)
    amp = np.array([[0.5, 1.0, 2.0, 0.25], [1.5, 0.1, 0.7, 3.0], [0.05, 0.9, 1.1, 0.6]])  # per antenna and 1000 samples
    z = (rng.standard_normal((3, R1)) + 1j * rng.standard_normal((3, R1))) * amp[:, np.arange(R1) // 1000]
    return z.astype(np.complex64)


def _np_scan(z, R, end, length, n_partial, n_ant):
    n_ant = min(n_ant, z.shape[0])
    start = end - (n_partial * length - 1)
    out = []
    for p in range(n_partial):
        idx = (start + p * length + np.arange(length)) % R
        e = np.sum(np.abs(z[:n_ant, idx].astype(np.complex128)) ** 2)
        out.append(np.sqrt(e / (length * n_ant)))
    return np.array(out)


def test_chscan():
    import dnrp
    phy = _phy()
    z = _scan_ring()
    ring = _ring(3, STRIDE1)
    ring[:, :R1] = _dev(z)
    G = 7 * R1
    reqs = [dnrp.ChscanReq(G + 1999, 500, 3, 3),         # no wrap
            dnrp.ChscanReq(G + R1 + 99, 400, 3, 3),      # the third partial scan wraps
            dnrp.ChscanReq(G + R1 + 299, 300, 2, 3),     # the partial boundary is the ring end
            dnrp.ChscanReq(G + 2500, 700, 2, 1),
            dnrp.ChscanReq(G + 2900, 450, 4),            # N_ant unset (2^32 - 1): clamped to the ring's
            dnrp.ChscanReq(G + 5000, R1, 1, 2),          # one whole ring turn
            dnrp.ChscanReq(G + 1004, 2, 5, 3)]
    assert reqs[4].N_ant == 2 ** 32 - 1
    parts, avg = phy.chscan(ring, reqs, ring_len=R1)
    for i, q in enumerate(reqs):
        ref = _np_scan(z, R1, q.end, q.length, q.N_partial, q.N_ant)
        assert parts[i].shape == ref.shape
        err, err_avg = np.max(np.abs(parts[i] / ref - 1)), abs(avg[i] / ref.sum() - 1)
        print("chscan", i, err, err_avg)
        assert err < 1e-4 and err_avg < 1e-4, (i, err, err_avg)  # rms_avg: the sum, as chscan_t::rms_avg

    L = dnrp.lib()
    part, off, av = np.zeros(8, np.float32), np.zeros(1, np.uint32), np.zeros(1, np.float32)

    def call(req, ring_p=ring.data_ptr(), n_ant=3, req_null=False, out=(True, True, True)):
        return L.dnrp_chscan_batch(phy._ctx, ring_p, R1, STRIDE1, n_ant, 1, None if req_null else C.byref(req),
                                   part.ctypes.data if out[0] else None, off.ctypes.data if out[1] else None,
                                   av.ctypes.data if out[2] else None, None)

    ok = dnrp.ChscanReq(G + 999, 100, 4, 3)
    assert call(ok) == 0
    assert call(ok, ring_p=None) == -1 and call(ok, req_null=True) == -1
    for out in ((False, True, True), (True, False, True), (True, True, False)):
        assert call(ok, out=out) == -1
    assert call(ok, n_ant=0) == -1
    for q in (dnrp.ChscanReq(G + 999, 1, 4, 3), dnrp.ChscanReq(G + 999, 100, 0, 3), dnrp.ChscanReq(G + 999, 100, 4, 0),
              dnrp.ChscanReq(398, 100, 4, 3), dnrp.ChscanReq(-1, 100, 4, 3), dnrp.ChscanReq(G + 999, 1001, 3, 3)):
        assert call(q) == -1, (q.end, q.length, q.N_partial, q.N_ant)
    assert call(dnrp.ChscanReq(399, 100, 4, 3)) == 0  # start == 0

    # a span the virtual space just filled with noise alone: sqrt(n0) within half the variance bound
    S = 50000
    cfg = dnrp.ChannelCfg(dnrp.CH_AWGN, 0, 0.0, 0.0, 1, 1.0, 10.0, 0.8, 321)
    noise = _ring(2, S)
    phy.vspace_mix(cfg, [], None, noise, 3 * S + 77, S)
    parts, avg = phy.chscan(noise, [dnrp.ChscanReq(4 * S + 76, S // 2, 2)])
    n0 = 10 ** ((-10 * np.log10(0.8) - 10.0) / 10)
    print("noise rms", parts[0] / np.sqrt(n0))
    assert np.all(np.abs(parts[0] / np.sqrt(n0) - 1) < 0.015)
