"""The GPU turbo encoder and decoder (kernels/fec.hip, planned by csrc/host/fec.cpp) against their host
twins over every code-block size and the paths no other test reaches -- inputs of tests/fec_size_cases.py,
the host side of which tests/test_fec_sizes_host.py holds to the numpy oracle:

  - fec_encode_kernel / fec_pack_kernel for all 188 K x 4 rv x 3 rate classes, direct and packed stores;
  - fec_dematch_kernel / fec_tdec_kernel for every K with 1 and 3 active lanes of 64;
  - the continuation pass with a full second wave of one size (fec_compact_kernel over several
    source waves);
  - saturated soft bits, one-shot and combined over four transmissions, with the softbuffer read back;
  - the false alarm's flag reset; fec_tbcrc_kernel's 1-KiB block edges on aligned and odd row strides.
Integer code with an exact host twin: verdicts, iteration counts and bytes are compared for equality.
Every device tensor is poisoned and wider than its longest row; nothing past a row's end may change
(d rows end at (G + 7) // 8, tb rows at N_TB_bits / 8 + 3)."""
import collections

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

D_POISON, TB_POISON, LLR_POISON, SB_POISON, FLAG_POISON = 0xAB, 0xEE, 32767, 0x5A5A, 0x77


def _mods():
    import dnrp
    import dnrp.fec as FE
    import fec_size_cases as S
    return dnrp, FE, S


def _dev():
    return torch.device("cuda:0")


def _rows(arrs, width, fill, dtype):
    out = np.full((len(arrs), width), fill, dtype)
    for i, a in enumerate(arrs):
        out[i, : len(a)] = a
    return out


def _encode_check(phy, FE, cfgs, tbs, tb_width=None):
    """dnrp_pdc_encode_batch of the packets against dnrp_pdc_encode, byte for byte, poison intact"""
    tb_width = tb_width or max(len(t) for t in tbs) + 1
    tb = torch.from_numpy(_rows(tbs, tb_width, 0xFF, np.uint8)).to(_dev())
    d = torch.full((len(cfgs), max((c.G + 7) // 8 for c in cfgs) + 5), D_POISON, dtype=torch.uint8, device=_dev())
    assert tb.data_ptr() % 16 == 0   # row 0 is 16-byte aligned, the others by their stride
    FE.pdc_encode_batch(phy, cfgs, tb, d)
    g = d.cpu().numpy()
    for i, c in enumerate(cfgs):
        ref = FE.pdc_encode(c, tbs[i])
        assert len(ref) == (c.G + 7) // 8
        assert (g[i, : len(ref)] == ref).all(), (i, c.N_TB_bits, c.N_bps, c.G, c.rv,
                                                 int(np.flatnonzero(g[i, : len(ref)] != ref)[0]))
        assert (g[i, len(ref):] == D_POISON).all(), (i, c.N_TB_bits, c.G, "bytes past the row's end")
    return g


def _decode_check(phy, FE, packets, want=None, tb_width=None):
    """dnrp_pdc_decode_batch of [(cfg, tb, llr)] against dnrp_pdc_decode per packet -> host results"""
    cfgs = [p[0] for p in packets]
    want = want or [FE.pdc_decode(c, l) for c, _, l in packets]
    llr = torch.from_numpy(_rows([p[2] for p in packets], max(c.G for c in cfgs) + 5, LLR_POISON, np.int16)).to(_dev())
    tb_width = tb_width or max(c.N_TB_bits for c in cfgs) // 8 + 3 + 7
    tb = torch.full((len(cfgs), tb_width), TB_POISON, dtype=torch.uint8, device=_dev())
    assert tb.data_ptr() % 16 == 0
    ok, it = FE.pdc_decode_batch(phy, cfgs, llr, tb)
    _compare_decode(FE, cfgs, [p[1] for p in packets], ok, it, tb.cpu().numpy(), want)
    return want


def _compare_decode(FE, cfgs, sent, ok, it, g_tb, want):
    for i, (c, (h_ok, h_tb, h_it)) in enumerate(zip(cfgs, want)):
        nb = c.N_TB_bits // 8
        assert (bool(ok[i]), int(it[i])) == (h_ok, h_it), (i, c.N_TB_bits, c.N_bps, c.G, c.rv, ok[i], it[i], h_ok, h_it)
        assert (g_tb[i, :nb] == h_tb).all(), (i, c.N_TB_bits, c.N_bps, c.G, c.rv)
        assert (g_tb[i, nb + 3:] == TB_POISON).all(), (i, c.N_TB_bits, "bytes past the row's end")
        if h_ok:
            assert (h_tb == sent[i]).all()
            crc = FE.crc(h_tb, c.N_TB_bits, FE.CRC24A)
            assert list(g_tb[i, nb: nb + 3]) == [crc >> 16, (crc >> 8) & 255, crc & 255], (i, "CRC24A after the TB")


def test_gpu_encoder_every_size_direct_mode(monkeypatch):
    """The grid cases whose G is a whole number of bytes (every Qm = 8 case among them) in one batch:
    fec_encode_kernel stores into the d rows itself, no fec_pack launch."""
    dnrp, FE, S = _mods()
    monkeypatch.setenv("DNRP_TIMING", "1")
    phy = dnrp.Phy(1, 1, 1, max_batch=1)
    grid = S.size_grid()
    pick = [n for n, g in enumerate(grid) if g[4] % 8 == 0]
    assert {grid[n][0] for n in pick} == set(S.SIZES) and all(grid[n][4] % 8 == 0 for n in pick)
    assert {(grid[n][1], grid[n][2]) for n in pick} == {(rv, rc) for rv in range(4) for rc in range(3)}
    assert sum(grid[n][3] == 8 for n in pick) == sum(g[3] == 8 for g in grid) > 400
    cfgs = [FE.fec_cfg(grid[n][0] - 24, grid[n][3], grid[n][4], rv=grid[n][1]) for n in pick]
    _encode_check(phy, FE, cfgs, [S.grid_tb(n, grid[n][0]) for n in pick])
    assert phy.kernel_time_total("fec_pack")[1] == 0 and phy.kernel_time_total("fec_encode")[1] > 0
    phy.close()


def test_gpu_encoder_every_size_packed_mode(monkeypatch):
    """All 188 x 4 x 3 grid cases and the C > 1 packets with two block lengths in one batch: the packed
    scratch and fec_pack_kernel, block starts inside a byte."""
    dnrp, FE, S = _mods()
    monkeypatch.setenv("DNRP_TIMING", "1")
    phy = dnrp.Phy(1, 1, 1, max_batch=1)
    grid = S.size_grid()
    cfgs = [FE.fec_cfg(K - 24, Qm, G, rv=rv) for K, rv, rc, Qm, G in grid]
    tbs = [S.grid_tb(n, g[0]) for n, g in enumerate(grid)]
    for n, (t, Qm, G, rv) in enumerate(S.PACK_EXTRAS):
        E = S.cb_E(t, Qm, G)
        assert any(sum(E[:r]) % 8 for r in range(len(E))), (t, Qm, G)
        cfgs.append(FE.fec_cfg(t, Qm, G, rv=rv))
        tbs.append(S.grid_tb(10000 + n, t + 24))
    _encode_check(phy, FE, cfgs, tbs)
    assert phy.kernel_time_total("fec_pack")[1] > 0 and phy.kernel_time_total("fec_encode")[1] > 0
    phy.close()


def test_gpu_decoder_every_size():
    """One packet per K in one call (every wave holds one active lane and 63 inactive ones), then three
    noise draws per K (three active lanes): verdict, iterations and bytes of the host per packet."""
    dnrp, FE, S = _mods()
    phy = dnrp.Phy(1, 1, 1, max_batch=1)
    n = len(S.SIZES)
    one = [S.sweep_packet(i) for i in range(n)]
    want = _decode_check(phy, FE, one)
    hist = collections.Counter((ok, it) for ok, _, it in want)
    assert hist[(True, 2)] >= 10 and hist[(False, 10)] >= 10 and sum(v for (o, i), v in hist.items() if o and i >= 4) >= 10
    three = [S.sweep_packet(i, rep=r) for i in range(n) for r in range(3)]
    want3 = _decode_check(phy, FE, three)
    assert [w[2] for w in want3[::3]] == [w[2] for w in want]
    phy.close()


def test_gpu_decoder_continuation_full_second_wave():
    """More than 64 blocks of one size still undecided after the first three iterations: run_tdec opens a
    second dense wave of the same K, fec_compact_kernel gathers lanes out of three source waves. Host
    counts with these inputs: K = 256: 96 of 160 undecided, 64 decided, 58 failing; K = 264: 49 of 70
    undecided, 21 decided, 26 failing."""
    dnrp, FE, S = _mods()
    phy = dnrp.Phy(1, 1, 1, max_batch=1)
    pk = S.cont_packets()
    want = [FE.pdc_decode(c, l) for c, _, l in pk]
    stats = {}
    for (c, _, _), (ok, _, it) in zip(pk, want):
        s = stats.setdefault(c.N_TB_bits + 24, collections.Counter())
        s["undecided" if it > 3 else "decided"] += 1
        s["failing"] += not ok
    print("continuation counts per K:", {K: dict(v) for K, v in stats.items()})
    assert set(stats) == {K for K, _ in S.CONT_SIZES}
    assert any(s["undecided"] > 64 and s["decided"] >= 20 for s in stats.values()), stats
    _decode_check(phy, FE, pk, want=want)
    phy.close()


def test_gpu_saturated_soft_bits_one_shot():
    """+32767 / -32768 soft bits repeated 2.2 to 15 times (K = 40, Qm = 1): fec_dematch_kernel clamps
    after every add as rm_rx does; tests/test_fec_sizes_host.py shows that these inputs reach the clamp
    and that clamping the plain sum once gives other buffers."""
    dnrp, FE, S = _mods()
    phy = dnrp.Phy(1, 1, 1, max_batch=1)
    pk = S.sat_oneshot()
    n_order = 0
    for c, _, llr in pk:
        K = c.N_TB_bits + 24
        plain = S.unclamped_sums(llr, K, c.rv)
        n_order += int((np.clip(plain, -32768, 32767) != S.ON.rate_dematch(llr, K, c.rv)).sum())
    assert n_order > 0 and max(c.G / (3 * (c.N_TB_bits + 28)) for c, _, _ in pk) >= 14.9
    want = _decode_check(phy, FE, pk)
    out = [(ok, it) for ok, _, it in want]
    assert (True, 2) in out and any(ok and it > 3 for ok, it in out) and any(not ok for ok, _ in out)
    phy.close()


def test_gpu_saturated_soft_bits_harq():
    """Four saturated transmissions (rv 0, 2, 3, 1) through dnrp_pdc_decode_batch_harq against the host
    with a dnrp_harq_rx per packet after every rv; the device softbuffer ([stream][K + 4] per block)
    against fec_np.rate_dematch accumulated over the transmissions of a block until it has passed."""
    dnrp, FE, S = _mods()
    phy = dnrp.Phy(1, 1, 1, max_batch=1)
    m = len(S.SAT_HARQ)
    Ks = [S.SAT_CASES[n][0] for n, _ in S.SAT_HARQ]
    ent = [FE.softbuffer_size(K - 24)[0] for K in Ks]
    assert ent == [3 * (K + 4) for K in Ks]
    sb_h = np.full((m, max(ent) + 9), SB_POISON, np.int16)
    fl_h = np.full((m, 4), FLAG_POISON, np.uint8)
    for i in range(m):
        sb_h[i, : ent[i]] = 0
        fl_h[i, 0] = 0
    sb, flags = torch.from_numpy(sb_h).to(_dev()), torch.from_numpy(fl_h).to(_dev())
    tb = torch.full((m, max(Ks) // 8 + 7), TB_POISON, dtype=torch.uint8, device=_dev())
    hbs = [FE.HarqRx(K - 24) for K in Ks]
    w = [None] * m
    done = [False] * m
    first = last = None
    plain = [None] * m
    for rv in S.HARQ_RVS:
        pk = [S.sat_packet(n, rv=rv, flip=fl, draw=1) for n, fl in S.SAT_HARQ]
        cfgs = [p[0] for p in pk]
        llr = torch.from_numpy(_rows([p[2] for p in pk], max(c.G for c in cfgs) + 5, LLR_POISON, np.int16)).to(_dev())
        ok, it = FE.pdc_decode_batch_harq(phy, cfgs, llr, sb, flags, tb)
        want = [FE.pdc_decode(c, l, hbs[i]) for i, (c, _, l) in enumerate(pk)]
        _compare_decode(FE, cfgs, [p[1] for p in pk], ok, it, tb.cpu().numpy(), want)
        g_sb, g_fl = sb.cpu().numpy(), flags.cpu().numpy()
        for i, (c, _, l) in enumerate(pk):
            if not done[i]:  # a block that has passed is not combined any more
                w[i] = S.ON.rate_dematch(l, Ks[i], rv, w[i])
                plain[i] = S.unclamped_sums(l, Ks[i], rv, plain[i])
                done[i] = want[i][0]
            ref = S.ON._streams(w[i], Ks[i]).reshape(-1)
            assert (g_sb[i, : ent[i]] == ref).all(), (rv, i, Ks[i], int(np.flatnonzero(g_sb[i, : ent[i]] != ref)[0]))
            assert (g_sb[i, ent[i]:] == np.int16(SB_POISON)).all(), (rv, i, "softbuffer past the row's end")
            assert g_fl[i, 0] == int(done[i]) and (g_fl[i, 1:] == FLAG_POISON).all(), (rv, i, g_fl[i])
        first = first if first is not None else [x[0] for x in want]
        last = [x[0] for x in want]
    n_clamped = sum(int((np.abs(p) > 32767).sum()) for p in plain)
    assert n_clamped > 0
    assert any(not a and b for a, b in zip(first, last)) and any(first) and not all(last)
    phy.close()


def test_gpu_false_alarm_resets_flags():
    """Every code-block CRC24B right, the transport-block CRC24A wrong: the packet's HARQ flags are
    cleared, so the next call decodes every block again; correct packets keep flags and bytes."""
    dnrp, FE, S = _mods()
    phy = dnrp.Phy(1, 1, 1, max_batch=1)
    tbs, Qm, G, rv = S.FALSE_ALARM
    d, tb_bits = S.false_alarm_bits(tbs, Qm, G, rv)
    cfgs = [FE.fec_cfg(tbs, Qm, G, rv=rv)]
    llrs, sent = [S.clean_llr(d)], [np.packbits(tb_bits)]
    for n, (t, q, g, r) in enumerate((S.CORRECT_MULTI, S.CORRECT_SINGLE)):
        cfgs.append(FE.fec_cfg(t, q, g, rv=r))
        sent.append(S.grid_tb(20000 + n, t + 24))
        llrs.append(S.clean_llr(np.unpackbits(FE.pdc_encode(cfgs[-1], sent[-1]))[:g]))
    m = 3
    sizes = [FE.softbuffer_size(c.N_TB_bits) for c in cfgs]
    Cs = [s[1] for s in sizes]
    assert Cs[0] > 1 and Cs[1] > 1 and Cs[2] == 1
    sb_h = np.full((m, max(s[0] for s in sizes) + 9), SB_POISON, np.int16)
    fl_h = np.full((m, max(Cs) + 3), FLAG_POISON, np.uint8)
    for i in range(m):
        sb_h[i, : sizes[i][0]] = 0
        fl_h[i, : Cs[i]] = 0
    sb, flags = torch.from_numpy(sb_h).to(_dev()), torch.from_numpy(fl_h).to(_dev())
    llr = torch.from_numpy(_rows(llrs, max(c.G for c in cfgs) + 5, LLR_POISON, np.int16)).to(_dev())
    tb = torch.full((m, max(c.N_TB_bits for c in cfgs) // 8 + 3 + 7), TB_POISON, dtype=torch.uint8, device=_dev())
    hbs = [FE.HarqRx(c.N_TB_bits) for c in cfgs]
    g_first = None
    for call in range(2):
        ok, it = FE.pdc_decode_batch_harq(phy, cfgs, llr, sb, flags, tb)
        want = [FE.pdc_decode(c, l, hbs[i]) for i, (c, l) in enumerate(zip(cfgs, llrs))]
        g_tb, g_fl, g_sb = tb.cpu().numpy(), flags.cpu().numpy(), sb.cpu().numpy()
        assert (bool(ok[0]), int(it[0])) == (False, 2 * Cs[0]) == (want[0][0], want[0][2]), (call, ok[0], it[0])
        assert (g_fl[0, : Cs[0]] == 0).all(), (call, g_fl[0])
        for i in (1, 2):
            assert (bool(ok[i]), int(it[i])) == (True, 2 * Cs[i] if call == 0 else 0) == (want[i][0], want[i][2]), (call, i)
            assert (g_fl[i, : Cs[i]] == 1).all(), (call, i, g_fl[i])
        for i in range(m):
            nb = cfgs[i].N_TB_bits // 8
            assert (g_tb[i, :nb] == want[i][1]).all() and (g_tb[i, :nb] == sent[i]).all(), (call, i)
            assert (g_tb[i, nb + 3:] == TB_POISON).all(), (call, i)
            assert (g_fl[i, Cs[i]:] == FLAG_POISON).all() and (g_sb[i, sizes[i][0]:] == np.int16(SB_POISON)).all(), (call, i)
        if call == 0:
            g_first = g_tb.copy()
        else:
            assert (g_tb == g_first).all()
    phy.close()


@pytest.mark.parametrize("stride", [5152, 5151], ids=["rows_16B_aligned", "rows_odd"])
def test_gpu_tbcrc_block_edges(stride):
    """Transport blocks of 1023, 1039, 5120 and 5136 bytes (1023, 15, 0 and 16 mod fec_tbcrc_kernel's
    1-KiB block) through the encoder (CRC24A computed) and the decoder (CRC24A checked), on tb rows
    whose stride is a multiple of 16 (whole pieces take the 16-byte load) and odd (rows 1 ... are
    misaligned: the byte path). One TB byte flipped: another CRC, other d-bits."""
    dnrp, FE, S = _mods()
    phy = dnrp.Phy(1, 1, 1, max_batch=1)
    t, q, g, r = S.CORRECT_SINGLE   # row 0, the only row an odd stride leaves aligned
    c0 = FE.fec_cfg(t, q, g, rv=r)
    tb0 = S.grid_tb(20001, t + 24)
    pk = [(c0, tb0, S.clean_llr(np.unpackbits(FE.pdc_encode(c0, tb0))[:g]))]
    pk += [S.tbcrc_packet(nb, n) for n, nb in enumerate(S.TBCRC_BYTES)]
    assert [len(p[1]) % 1024 for p in pk[1:]] == [1023, 15, 0, 16]
    assert [FE.cbsegm(p[0].N_TB_bits, S.Z)["C"] for p in pk[1:]] == [2, 2, 7, 7]
    cfg_f, tb_f, _ = pk[-1]
    flipped = tb_f.copy()
    flipped[1040] ^= 0x10
    assert FE.crc(flipped, cfg_f.N_TB_bits, FE.CRC24A) != FE.crc(tb_f, cfg_f.N_TB_bits, FE.CRC24A)
    cfgs = [p[0] for p in pk] + [cfg_f]
    assert stride >= max(c.N_TB_bits for c in cfgs) // 8 + 3
    g_d = _encode_check(phy, FE, cfgs, [p[1] for p in pk] + [flipped], tb_width=stride)
    assert (g_d[-1] != g_d[-2]).any()
    # the decode of the unflipped soft bits passes with the unflipped bytes, on the same row stride
    want = _decode_check(phy, FE, pk, tb_width=stride)
    assert all(ok for ok, _, _ in want)
    assert [it for _, _, it in want] == [2 * FE.cbsegm(p[0].N_TB_bits, S.Z)["C"] for p in pk]
    phy.close()
