"""Sync parity at window edges, antenna gates and unaligned layouts: dnrp_rx_sync_batch / dnrp_rx_sync_stream
(kernels/sync_*.hip) against the oracle on the windows of tests/sync_edge_cases.py, whose branch coverage and
margins tests/test_sync_edges_host.py proves from the oracle alone.

Per case: the report count is the oracle's, every report passes test_gpu_sync.py's _compare (no tolerance is new),
the slots past the count are not found, and every report is a transmitted packet (fine peak = its start, its
N_eff_TX).
 - position    packets at the head (ignore_before) and the tail (search_len) of the search, every step-sum form
 - truncation  windows shorter than what the kernels read: step sums, fine stage, coarse range, the STF itself;
               odd S_win; noise-free tails of exactly zero power; inline and split-round peak searches
 - gates       antennas below rms_min, above SYNC_RMS_MAX, exactly silent: detection_ant_idx moves on, a silent
               antenna has coarse_peak_array = rms_array = 0.0 exactly, nothing is NaN or Inf, its rows of the
               sync_fine_peaks table are zero (it is not searched) and its row of the sync_icfo_scores table is
               0.0 in every searched column (sync_icfo_kernel transforms every searched antenna of a found report:
               a silent antenna's spectrum is zero), -1 elsewhere; N_ant_limited = 2 of 4 sees antennas 0, 1 only
 - layout      a base pointer 8 bytes into a 16-byte unit, odd S_win, overlapping windows over one linear stream
               (win_stride = chunk_len), padded antenna rows: reports equal the plain layout's (_check_equal)
 - stream      one packet swept across a chunk boundary of rx_sync_stream, in one call and in two calls split at
               that boundary: reported once, at its time, by the chunk the oracle + baton restatement names
 - backtoback  a second STF right behind skip_after_peak, and two packets overlapping in time
 - chain       a cut window and a silent-antenna window through rx_pcc_batch / rx_pdc_batch
Each test prints its largest deviation per toleranced field.
"""
import collections
import functools

import numpy as np
import pytest

import llr_gate
import oracle_py as O
import phy_fixtures as F
import sync_edge_cases as E
from test_gpu_stream import _oracle_stream
from test_gpu_sync import _compare, _phy, _run
from test_gpu_sync_tranche import _check_equal

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FLOAT_FIELDS = ("detection_rms", "detection_metric", "coarse_peak_array", "rms_array", "cfo_fractional_rad",
                "cfo_integer_rad", "fine_peak_metric")


class Worst(dict):
    """largest deviation per toleranced field over the reports a test compared"""

    def add(self, g, o):
        nt = int(np.count_nonzero(o["xc_metric"]))
        rel = lambda x, y: float(np.max(np.abs(np.asarray(x, np.float64) - y) / np.maximum(np.abs(y), 1e-30), initial=0.0))
        live = o["coarse_metric"] > 0
        for k, v in (("coarse_peak_time_local [samples]", abs(int(g["coarse_peak_time_local"]) - o["coarse_local"])),
                     ("cfo_fractional_rad [abs]", abs(float(g["cfo_fractional_rad"]) - o["cfo_frac"])),
                     ("detection_metric [rel]", rel(g["detection_metric"], o["det_metric"])),
                     ("coarse_peak_array [rel]", rel(g["coarse_peak_array"][live], o["coarse_metric"][live])),
                     ("rms_array [rel]", rel(g["rms_array"][live], o["rms"][live])),
                     ("fine_peak_metric [rel]", rel(g["fine_peak_metric"][:nt], o["xc_metric"][:nt]))):
            self[k] = max(self.get(k, 0.0), v)

    def show(self, what):
        print(what, "largest deviations:", ", ".join("%s %.3g" % kv for kv in self.items()))


def _env(monkeypatch, env):
    for k in ("DNRP_SYNC_PIPE", "DNRP_SYNC_STREAM", "DNRP_SYNC_ROUNDS", "DNRP_SYNC_TRANCHE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _sync_cfg(c):
    import dnrp
    psd, cfgt = F.case(c.name)
    return dnrp.SyncCfg(psd[0], psd[1], c.n_lim or cfgt[2], c.chunk, c.max_reports)


def _finite(res, cnt, where):
    for w in range(res.shape[0]):
        for k in range(int(cnt[w])):
            for f in FLOAT_FIELDS:
                assert np.all(np.isfinite(res[w, k][f])), (where, w, k, f, res[w, k][f])


def _check_cases(cases, res, cnt, where, worst):
    """the per-case gates of the module docstring; res [len(cases), max_reports]"""
    _finite(res, cnt, where)
    for w, c in enumerate(cases):
        ref = E.oracle(c)[0]
        assert int(cnt[w]) == len(ref), (where, c.id, int(cnt[w]), [r["fine_64"] for r in ref])
        for k, o in enumerate(ref):
            _compare(res[w, k], o, (where, c.id, k))
            worst.add(res[w, k], o)
            assert int(res[w, k]["fine_peak_time"]) in c.starts and int(res[w, k]["N_eff_TX"]) == E.n_eff_tx(c), (where, c.id)
            dead = o["coarse_metric"][:F.case(c.name)[1][2]] == 0  # antennas the oracle leaves invalid: exact zeros
            n = len(dead)
            assert np.all(res[w, k]["coarse_peak_array"][:n][dead] == 0.0) and np.all(res[w, k]["rms_array"][:n][dead] == 0.0), \
                (where, c.id, res[w, k]["coarse_peak_array"], res[w, k]["rms_array"])
        for k in range(len(ref), c.max_reports):
            assert int(res[w, k]["found"]) == 0, (where, c.id, k)


def _run_group(cases, phy=None, max_batch=32):
    """one call for cases of one configuration, S_win, N_ant_limited and max_reports"""
    c0 = cases[0]
    assert all((c.name, c.S_win, c.n_lim, c.max_reports, c.chunk) == (c0.name, c0.S_win, c0.n_lim, c0.max_reports, c0.chunk)
               for c in cases)
    phy = phy or _phy(c0.name, max_batch=max_batch)
    return _run(phy, _sync_cfg(c0), [E.window(c)[0] for c in cases], c0.max_reports)


def _forms(names):
    return [(n, i) for n in names for i in range(len(E.FORMS[n]))]


def _form_id(v):
    return v if isinstance(v, str) else "form%d" % v


# ---------------------------------------------------------------- position
@pytest.mark.parametrize("name,form", _forms(["C2", "C3", "os2_u2b2_tm1"]), ids=_form_id)
def test_position(name, form, monkeypatch):
    _env(monkeypatch, E.FORMS[name][form])
    cases = [c for c in E.POSITION if c.name == name]
    res, cnt = _run_group(cases)
    worst = Worst()
    _check_cases(cases, res, cnt, ("position", E.FORMS[name][form]), worst)
    assert {int(n) for n in cnt} == {0, 1}  # both outcomes in the batch
    worst.show("position %s %s" % (name, E.FORMS[name][form]))


# ---------------------------------------------------------------- truncation
@pytest.mark.parametrize("name,form", _forms(["C2", "C3", "lm1_1_u8b16", "lm40_27_u8b12_tm5", "os2_u2b2_tm1"]), ids=_form_id)
def test_truncation(name, form, monkeypatch):
    _env(monkeypatch, E.FORMS[name][form])
    phy = _phy(name)
    worst = Worst()
    by_size = collections.defaultdict(list)
    for c in E.TRUNCATION:
        if c.name == name:
            by_size[c.S_win].append(c)
    assert len(by_size) >= 8
    for S_win, cases in sorted(by_size.items(), reverse=True):  # every S_win is a call of its own
        res, cnt = _run_group(cases, phy)
        _check_cases(cases, res, cnt, ("truncation", E.FORMS[name][form], S_win), worst)
    worst.show("truncation %s %s" % (name, E.FORMS[name][form]))


# ---------------------------------------------------------------- antenna gates
def _gate_groups(name):
    g = collections.defaultdict(list)
    for c in E.GATES:
        if c.name == name:
            g[(c.S_win, c.n_lim)].append(c)
    return list(g.values())


@pytest.mark.parametrize("name", ["tm1_txdiv2", "mrc4_16qam"])
def test_gates(name):
    phy = _phy(name)
    worst = Worst()
    moved = 0
    for cases in _gate_groups(name):
        res, cnt = _run_group(cases, phy)
        _check_cases(cases, res, cnt, "gates", worst)
        for w, c in enumerate(cases):
            if c.gains is not None and c.gains[0] != 1.0:  # antenna 0 gated: the detection is another antenna's
                assert int(res[w, 0]["detection_ant_idx"]) != 0, c.id
                moved += 1
            if c.kind in ("gate_zero", "gate_one_live"):
                silent = [a for a, x in enumerate(c.gains) if x == 0.0]
                assert np.all(res[w, 0]["coarse_peak_array"][silent] == 0.0) and np.all(res[w, 0]["rms_array"][silent] == 0.0)
    assert moved >= 3
    worst.show("gates %s" % name)


@pytest.mark.parametrize("name", ["tm1_txdiv2", "mrc4_16qam"])
def test_gates_silent_antenna_all_antenna_fine_search(name):
    """set_sync_fine_all_antennas(1): the silent antenna has no coarse peak and is not searched (its table rows are
    zero), the others are; the report is still the transmitted packet"""
    phy = _phy(name)
    phy.set_sync_fine_all_antennas(1)
    n_ant = F.case(name)[1][2]
    for cases in _gate_groups(name):
        cases = [c for c in cases if c in E.GATES_ZERO]
        if not cases:
            continue
        res, cnt = _run_group(cases, phy)
        metric, index = phy.sync_fine_peaks(len(cases) * cases[0].max_reports)
        _finite(res, cnt, "fine_all")
        assert np.all(np.isfinite(metric))
        for w, c in enumerate(cases):
            o = E.oracle(c)[0][0]
            assert int(cnt[w]) == 1 and int(res[w, 0]["fine_peak_time"]) == c.starts[0], (c.id, res[w, 0])
            assert int(res[w, 0]["N_eff_TX"]) == E.n_eff_tx(c) and int(res[w, 0]["detection_ant_idx"]) == o["det_ant"], c.id
            rows = metric[w * c.max_reports]
            for a in range(8):
                valid = a < n_ant and o["coarse_metric"][a] > 0
                assert bool(rows[a].any()) == valid and bool(index[w * c.max_reports, a].any()) <= valid, (c.id, a, rows[a])
            assert not metric[w * c.max_reports + 1].any()  # the slot that is not found


def test_gates_silent_antenna_icfo_scores():
    """set_sync_icfo_search(1): sync_icfo_kernel transforms every searched antenna of a found report, the silent one
    included; its samples are zero through any resampler, so its score is exactly 0.0 in every column the live
    antenna has a score in and -1 elsewhere. The decision is k = 0 and the report the oracle's."""
    c = E.BY_ID[E.GATES_ICFO]
    phy = _phy(c.name)
    phy.set_sync_icfo_search(1)
    res, cnt = _run_group([c], phy)
    score, k = phy.sync_icfo_scores(c.max_reports)
    worst = Worst()
    _check_cases([c], res, cnt, "icfo", worst)
    assert np.all(np.isfinite(score)) and int(k[0]) == 0 and float(res[0, 0]["cfo_integer_rad"]) == 0.0
    silent, live = score[0, 0], score[0, 1]
    assert np.array_equal(live == -1, [True, True, True, False, False, False, True, True, True]), live
    assert np.all(live[3:6] > 0) and np.array_equal(silent, np.where(live == -1, -1.0, 0.0).astype(np.float32)), (silent, live)
    assert np.all(score[0, 2:] == -1) and np.all(score[1:] == -1)  # unsearched antennas, the slot that is not found
    worst.show("icfo")


# ---------------------------------------------------------------- layout
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(*a.shape, 2)).to("cuda:0")


JUNK = np.complex64(100 + 100j)  # between rows: far above SYNC_RMS_MAX, so a read of it shows


@pytest.mark.parametrize("layout", E.LAYOUTS)
@pytest.mark.parametrize("name", E.LAYOUT_NAMES)
def test_layout(name, layout):
    import dnrp
    psd, cfgt = F.case(name)
    n_ant, (S, chunk) = cfgt[2], E.SIZES[name]
    wins = np.stack(E.layout_windows(name))
    n = len(wins)
    phy = _phy(name, max_batch=32)
    sc = dnrp.SyncCfg(psd[0], psd[1], n_ant, chunk, 2)

    def plain(w, S_win=None):  # rows of an even length from a 16-byte aligned base
        t = _dev(w)
        assert t.data_ptr() % 16 == 0 and w.shape[2] % 2 == 0
        r, c = phy.rx_sync_batch(sc, t, w.shape[0], S_win or w.shape[2], n_ant * w.shape[2], w.shape[2])
        phy.sync()
        return r.copy(), c.copy()

    if layout == "offset1":
        res0, cnt0 = plain(wins)
        t = _dev(np.concatenate([np.full(1, JUNK), wins.reshape(-1)]))[1:]
        assert t.data_ptr() % 16 == 8
        res, cnt = phy.rx_sync_batch(sc, t, n, S, n_ant * S, S)
    elif layout == "odd":  # the baseline: the same S - 1 samples in rows of S, every row 16-byte aligned
        padded = wins.copy()
        padded[:, :, S - 1] = JUNK
        res0, cnt0 = plain(padded, S - 1)
        t = _dev(wins[:, :, :S - 1])
        res, cnt = phy.rx_sync_batch(sc, t, n, S - 1, n_ant * (S - 1), S - 1)
    elif layout == "overlap":  # window w = stream samples [w chunk, w chunk + S) of every antenna
        k = 5 if name == "C2" else 4
        stream = np.concatenate(list(wins[:k]), axis=1)  # [n_ant, k S]
        T = stream.shape[1]
        n_w = (T - S) // chunk + 1
        res0, cnt0 = plain(np.stack([stream[:, w * chunk:w * chunk + S] for w in range(n_w)]))
        assert n_w >= 16 and chunk < S and cnt0.sum() >= k
        t = _dev(stream)
        res, cnt = phy.rx_sync_batch(sc, t, n_w, S, chunk, T)
    else:  # pad3
        res0, cnt0 = plain(wins)
        padded = np.full((n, n_ant, S + 3), JUNK)
        padded[:, :, :S] = wins
        t = _dev(padded)
        res, cnt = phy.rx_sync_batch(sc, t, n, S, n_ant * (S + 3), S + 3)
    phy.sync()  # t stays alive until here
    _finite(res, cnt, layout)
    _check_equal((name, layout), res, cnt, res0, cnt0)
    assert cnt0.sum() >= 4 and 0 in cnt0
    if layout in ("offset1", "pad3"):  # and the plain run itself is the oracle's (test_position, default form)
        assert [int(x) for x in cnt0] == [len(E.oracle(c)[0]) for c in E.POSITION if c.name == name]


# ---------------------------------------------------------------- stream sweep
@functools.lru_cache(maxsize=None)
def _stream_phy():
    import dnrp
    phy = _phy("C2", max_batch=64)
    sc = dnrp.SyncCfg(1, 1, 1, E.STREAM_CHUNK, E.STREAM_MAX_REPORTS)
    assert phy.sync_stream_window(sc) == E.STREAM_S_WIN
    return phy, sc


@pytest.mark.parametrize("start", E.STREAM_STARTS)
def test_stream_sweep(start):
    phy, sc = _stream_phy()
    ring, g0 = E.stream_ring(start)
    osc = O.sync_cfg(1, 1, n_ant=1, chunk_len=E.STREAM_CHUNK)
    ref, dup = _oracle_stream(osc, ring, g0, E.STREAM_N_CHUNKS, E.STREAM_CHUNK, E.STREAM_S_WIN, E.STREAM_MAX_REPORTS,
                              E.STREAM_UNIQUE_LIMIT)
    assert [t - g0 for t, _, _ in ref] == [start]
    ring_d = _dev(ring)
    split = E.STREAM_BOUNDARY // E.STREAM_CHUNK
    for parts in ([(0, E.STREAM_N_CHUNKS)], [(0, split), (split, E.STREAM_N_CHUNKS - split)]):
        state = phy.sync_stream_init(sc)
        assert state.sync_time_unique_limit == E.STREAM_UNIQUE_LIMIT
        got, chunk_of = [], []
        for first, n in parts:  # the state carries the baton from call to call
            res, ck = phy.rx_sync_stream(sc, ring_d, g0 + first * E.STREAM_CHUNK, n, state)
            got += list(res)
            chunk_of += [int(k) + first for k in ck]
        assert [int(g["fine_peak_time"]) - g0 for g in got] == [start], (start, parts)  # once, at its time
        assert chunk_of == [ref[0][1]] and int(state.not_unique) == dup and int(state.packets) == 1, (start, parts, chunk_of)
        assert int(got[0]["N_eff_TX"]) == ref[0][2]["N_eff_TX"]
        assert abs(float(got[0]["cfo_fractional_rad"]) - ref[0][2]["cfo_frac"]) < 2e-6


# ---------------------------------------------------------------- back to back
@pytest.mark.parametrize("rounds", [None, "0", "2"])
def test_back_to_back(rounds, monkeypatch):
    _env(monkeypatch, {} if rounds is None else {"DNRP_SYNC_ROUNDS": rounds})
    res, cnt = _run_group(E.BACKTOBACK)
    worst = Worst()
    _check_cases(E.BACKTOBACK, res, cnt, ("backtoback", rounds), worst)
    assert [int(n) for n in cnt][:4] == [2, 2, 2, 2]
    worst.show("back to back, rounds %s" % rounds)


# ---------------------------------------------------------------- chain
@pytest.mark.parametrize("cid", E.CHAIN)
def test_chain(cid):
    """GPU sync -> GPU PCC / PDC on the edge window against the oracle RX fed the GPU report (test_sync_then_demodulate):
    LLRs within the gate, every hard decision the transmitted bit"""
    import dnrp
    c = E.BY_ID[cid]
    psd, cfgt = F.case(c.name)
    lr = F.PARITY_CASES[c.name][2] if c.name in F.PARITY_CASES else 1
    win, meta = E.window(c)
    phy = _phy(c.name)
    ps = dnrp.psdef(*psd)
    sz = phy.packet_sizes(ps)
    assert c.starts[0] + sz["N_samples_packet_os_rs"] <= c.S_win  # the packet is whole
    res, cnt = _run_group([c], phy)
    worst = Worst()
    _check_cases([c], res, cnt, "chain", worst)
    iq = _dev(win[None])
    reps = dnrp.sync_reports(res[:, 0])
    pcc_llr = torch.zeros((1, 196), dtype=torch.int16, device="cuda:0")
    pdc_llr = torch.zeros((1, sz["G"]), dtype=torch.int16, device="cuda:0")
    phy.rx_pcc_batch(reps, iq, pcc_llr)
    phy.rx_pdc_batch([dnrp.PdcReq(ps, 0, meta[0][2], meta[0][3])], iq, pdc_llr)
    phy.sync()
    g_pcc, g_pdc = pcc_llr.cpu().numpy()[0], pdc_llr.cpu().numpy()[0]
    ocf = O.cfg(cfgt[0], cfgt[1], os_min=cfgt[3], L=cfgt[4], M=cfgt[5], lr=lr)
    r = O.rx(ocf, O.psdef(*psd), win, int(res[0, 0]["fine_peak_time"]), float(res[0, 0]["cfo_fractional_rad"]), meta[0][2],
             meta[0][3])
    llr_gate.check((cid, "pcc"), g_pcc, r["pcc_llr"])
    llr_gate.check((cid, "pdc"), g_pdc, r["pdc_llr"])
    assert np.array_equal(np.unpackbits(meta[0][1])[: sz["G"]], (g_pdc > 0).astype(np.uint8)), cid
    assert np.array_equal(np.unpackbits(meta[0][1])[: sz["G"]], (r["pdc_llr"] > 0).astype(np.uint8)), cid
    print(cid, "largest LLR difference: pcc", int(np.abs(g_pcc.astype(int) - r["pcc_llr"]).max()), "pdc",
          int(np.abs(g_pdc.astype(int) - r["pdc_llr"]).max()))
