"""Host channel coding over every code-block size (csrc/host/fec.cpp through the C-ABI) against the numpy
restatement of oracle/fec_np.py. The host code is the twin the GPU kernels are held to bit for bit
(tests/test_gpu_fec_sizes.py uses the same inputs, tests/fec_size_cases.py), so what is pinned here:

  - dnrp_pdc_encode == fec_np.pdc_encode for all 188 sizes K x 4 redundancy versions x 3 rate classes
    (punctured, exactly the circular buffer, repeated 2.6 times), the modulation order rotating;
  - dnrp_pdc_decode over every K at clean / marginal / just-below-threshold SNRs, with conditions on
    its own outcome histogram so the sweep holds 2-iteration stops, late stops and failures;
  - dnrp_pdc_decode == fec_np.pdc_decode (verdict, iterations, bits) on the sizes the numpy loops can
    afford: every K % 32 != 0 up to 512 and the sizes around each step change of the size table;
  - saturated soft bits (+32767 / -32768) repeated 2.2 to 15 times, one-shot and combined over four
    transmissions in a dnrp_harq_rx: the de-matcher's clamp after every add, checked to be reached;
  - the false alarm: all code-block CRCs right, transport-block CRC wrong -> the flags are reset.
All integer arithmetic: equality, no tolerance."""
import collections
import functools

import numpy as np
import pytest

dnrp = pytest.importorskip("dnrp")
import dnrp.fec as F  # noqa: E402

import fec_size_cases as S  # noqa: E402

ON = S.ON


def test_host_encoder_matches_numpy_every_size_rv_rate():
    grid = S.size_grid()
    assert len(grid) == 188 * 4 * 3 and {g[3] for g in grid} == set(S.QMS)
    for n, (K, rv, rc, Qm, G) in enumerate(grid):
        tb = S.grid_tb(n, K)
        d = F.pdc_encode(F.fec_cfg(K - 24, Qm, G, rv=rv), tb)
        ref = ON.pdc_encode(np.unpackbits(tb), S.Z, Qm, G, rv, S.qpp_of)
        assert np.array_equal(np.unpackbits(d)[:G], ref), (K, rv, rc, Qm, G)
        assert not np.unpackbits(d)[G:].any(), (K, rv, Qm, G, "pad bits of the last byte")
    # C > 1 with two lengths E and block starts inside a byte
    for n, (tbs, Qm, G, rv) in enumerate(S.PACK_EXTRAS):
        E = S.cb_E(tbs, Qm, G)
        assert len(set(E)) == 2 and any(sum(E[:r]) % 8 for r in range(len(E))), (tbs, Qm, G, E)
        tb = S.grid_tb(10000 + n, tbs + 24)
        d = F.pdc_encode(F.fec_cfg(tbs, Qm, G, rv=rv), tb)
        assert np.array_equal(np.unpackbits(d)[:G], ON.pdc_encode(np.unpackbits(tb), S.Z, Qm, G, rv, S.qpp_of))
    assert {Qm for _, Qm, _, _ in S.PACK_EXTRAS} == {1, 2, 6}


@functools.lru_cache(maxsize=None)
def _sweep():
    """host decode of the sweep: [(cfg, tb, llr, ok, decoded, iterations)] per size index"""
    out = []
    for i in range(len(S.SIZES)):
        cfg, tb, llr = S.sweep_packet(i)
        out.append((cfg, tb, llr) + F.pdc_decode(cfg, llr))
    return out


def test_host_decoder_every_size():
    """Measured with these inputs: 69 packets stop at 2 iterations, 25 / 17 / 15 / 5 / 6 / 3 / 5 / 1 pass
    after 3 ... 10, 42 fail at 10 (31 of them the punctured class at rv 1 and 2, which carries almost no
    systematic bits)."""
    res = _sweep()
    hist = collections.Counter((ok, it) for *_, ok, _, it in res)
    print("outcome histogram (ok, iterations): count", sorted(hist.items()))
    seen = collections.Counter()
    for i, (cfg, tb, llr, ok, dec, it) in enumerate(res):
        K, rv, rc, Qm, G, sc = S.sweep_case(i)
        assert 2 <= it <= 10 and (ok or it == 10), (K, ok, it)
        if ok:
            assert np.array_equal(dec, tb), (K, rv, rc, Qm)
        seen[(rv, rc, sc)] += 1
    assert len(seen) == 36, "every rv x rate class x SNR class is met"
    n_fail = sum(v for (ok, it), v in hist.items() if not ok)
    assert hist[(True, 2)] >= 10
    assert sum(v for (ok, it), v in hist.items() if ok and it >= 4) >= 10   # past the device's split
    assert hist[(False, 10)] >= 10 and n_fail == hist[(False, 10)]
    assert n_fail <= len(res) // 4, n_fail


def test_host_decoder_matches_numpy_on_small_and_edge_sizes():
    res = _sweep()
    cases = [(i, res[i][0], res[i][2], res[i][3:]) for i in S.numpy_subset()]
    for K in S.NUMPY_LARGE:
        i = S.SIZES.index(K)
        cfg, tb, llr = S.sweep_packet(i, snr_class=S.CLEAN)
        cases.append((i, cfg, llr, F.pdc_decode(cfg, llr)))
    ks = {S.SIZES[i] for i, *_ in cases}
    assert ks >= {40, 48, 504, 512, 528, 1008, 1024, 1056, 2048, 2112} and len(ks) == 45 + 7 + 3
    hist = collections.Counter()
    for i, cfg, llr, (ok_h, tb_h, it_h) in cases:
        ok_o, bits_o, it_o = ON.pdc_decode(llr, cfg.N_TB_bits, S.Z, cfg.N_bps, cfg.G, cfg.rv, S.qpp_of)
        assert (ok_h, it_h) == (bool(ok_o), it_o), (S.sweep_case(i), ok_h, it_h, ok_o, it_o)
        assert np.array_equal(np.unpackbits(tb_h), bits_o), S.sweep_case(i)
        hist[(ok_h, min(it_h, 4) if ok_h else it_h)] += 1
    print("subset outcomes (ok, iterations capped at 4 for passes): count", sorted(hist.items()))
    assert hist[(True, 2)] >= 5 and hist[(True, 4)] >= 5 and hist[(False, 10)] >= 5


def test_saturated_soft_bits_one_shot():
    """Soft bits at the int16 limits: the circular buffer's sums clamp after every add (rm_rx,
    fec_np.rate_dematch), so a sum that passes +32767 and then takes a -32768 ends at -1, not at the
    clamp of the plain sum. Host == numpy, and the inputs reach the clamp. Measured with these inputs:
    22571 plain sums beyond int16, 4519 buffer entries where clamping the plain sum once differs; 8
    packets pass at 2 iterations, 1 at 3, 1 at 4, 1 at 6, 17 fail at 10."""
    pk = S.sat_oneshot()
    n_clamped = n_order = 0
    outcomes = []
    for cfg, tb, llr in pk:
        K = cfg.N_TB_bits + 24
        assert set(np.unique(llr)) <= {-32768, 32767} and cfg.G >= 2.2 * 3 * (K + 4) - cfg.N_bps
        plain = S.unclamped_sums(llr, K, cfg.rv)
        w = ON.rate_dematch(llr, K, cfg.rv)
        n_clamped += int((np.abs(plain) > 32767).sum())
        n_order += int((np.clip(plain, -32768, 32767) != w).sum())
        ok_h, tb_h, it_h = F.pdc_decode(cfg, llr)
        if len(outcomes) < len(S.SAT_CASES):   # the first HARQ transmissions: test_saturated_soft_bits_harq
            ok_o, bits_o, it_o = S.np_decode_buffer(w, K)
            assert (ok_h, it_h) == (ok_o, it_o), (K, cfg.N_bps, cfg.G, cfg.rv, ok_h, it_h, ok_o, it_o)
            assert np.array_equal(np.unpackbits(tb_h), bits_o)
        if ok_h:
            assert np.array_equal(tb_h, tb)
        outcomes.append((ok_h, it_h))
    print("saturated one-shot outcomes", outcomes, "sums past int16:", n_clamped,
          "sums where clamping once differs:", n_order)
    assert max(c.G / (3 * (c.N_TB_bits + 28)) for c, _, _ in pk) >= 14.9   # K = 40, Qm = 1
    assert n_clamped > 0 and n_order > 0
    assert (True, 2) in outcomes and any(ok and it > 3 for ok, it in outcomes) and any(not ok for ok, _ in outcomes)


def test_saturated_soft_bits_harq():
    """The same over redundancy versions 0, 2, 3, 1 into one dnrp_harq_rx: the softbuffer saturates
    across transmissions. numpy twin: rate_dematch into the kept buffer until the block has passed.
    Measured: 2 of 11 packets pass after the first transmission, 10 after the fourth; 10353 plain sums
    beyond int16."""
    n_clamped = 0
    first, last = [], []
    for n, fl in S.SAT_HARQ:
        K = S.SAT_CASES[n][0]
        hb = F.HarqRx(K - 24)
        w, plain, done, kept = None, None, False, None
        for t, rv in enumerate(S.HARQ_RVS):
            cfg, tb, llr = S.sat_packet(n, rv=rv, flip=fl, draw=1)
            ok_h, tb_h, it_h = F.pdc_decode(cfg, llr, hb)
            if done:
                want = (True, kept, 0)
            else:
                plain = S.unclamped_sums(llr, K, rv, plain)
                w = ON.rate_dematch(llr, K, rv, w)
                want = S.np_decode_buffer(w, K)
                done, kept = want[0], want[1]
            assert (ok_h, it_h) == (want[0], want[2]), (n, fl, rv, ok_h, it_h, want[0], want[2])
            assert np.array_equal(np.unpackbits(tb_h), want[1]), (n, fl, rv)
            if ok_h:
                assert np.array_equal(tb_h, tb)
            (first if t == 0 else last if t == 3 else []).append(ok_h)
        n_clamped += int((np.abs(plain) > 32767).sum())
    print("HARQ passes after the first / fourth transmission:", sum(first), sum(last), "of", len(first),
          "sums past int16:", n_clamped)
    assert n_clamped > 0
    assert any(not a and b for a, b in zip(first, last)) and any(first) and not all(last)


def test_false_alarm_resets_the_code_block_flags():
    tbs, Qm, G, rv = S.FALSE_ALARM
    C = ON.cbsegm(tbs, S.Z)[0]
    d, tb_bits = S.false_alarm_bits(tbs, Qm, G, rv)
    cfg = F.fec_cfg(tbs, Qm, G, rv=rv)
    llr = S.clean_llr(d)
    assert C > 1
    ok_o, bits_o, it_o = ON.pdc_decode(llr, tbs, S.Z, Qm, G, rv, S.qpp_of)
    assert (bool(ok_o), it_o) == (False, 2 * C) and np.array_equal(bits_o, tb_bits)
    hb = F.HarqRx(tbs)
    for call in range(2):   # the flags were reset: every block is decoded again
        ok, tb, it = F.pdc_decode(cfg, llr, hb)
        assert (ok, it) == (False, 2 * C), (call, ok, it)
        assert np.array_equal(np.unpackbits(tb), tb_bits)
    # a correct block of several code blocks keeps its flags and its bytes
    tbs, Qm, G, rv = S.CORRECT_MULTI
    C = ON.cbsegm(tbs, S.Z)[0]
    assert C > 1
    cfg = F.fec_cfg(tbs, Qm, G, rv=rv)
    tb = S.grid_tb(20000, tbs + 24)
    llr = S.clean_llr(np.unpackbits(F.pdc_encode(cfg, tb))[:G])
    hb = F.HarqRx(tbs)
    for call, it_want in enumerate((2 * C, 0)):
        ok, got, it = F.pdc_decode(cfg, llr, hb)
        assert (ok, it) == (True, it_want) and np.array_equal(got, tb), (call, ok, it)
