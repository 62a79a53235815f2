"""The sync edge cases, host side (no GPU): the input proof of tests/test_gpu_sync_edges.py, from the oracle alone.

1. Branch trace: every case of tests/sync_edge_cases.py reaches the branch its kind names (oracle_py.sync_trace:
   steps ignored, RMS and front/back gate rejections per antenna, false alarms, "STF before the chunk" drops,
   antennas invalid at the coarse peak, fine-stage and resampler reads outside the window), and the kinds
   reached are the literal list KINDS: dropping a case's class fails here, before a GPU is asked.
2. Margin: the oracle's float and double paths agree on the report count, det_time, N_eff_TX and fine peak;
   another seed gives the same count; where nothing is reported no evaluated step's detection metric lies
   within 10 % of the threshold on an antenna inside the RMS gates. Cases that fail are taken out of the
   literal lists of sync_edge_cases.py, never skipped here; test_minimum_kept holds what must remain.
3. Wrong-kernel proofs, one per class: what a kernel that reads past S_win, ignores the RMS gates, searches
   the unsearched antennas, forgets ignore_before / search_len, or skips skip_after_peak would report differs
   from the oracle's report, so the GPU file's gates can tell.

The false-alarm branch (nvalid == 0) and the "STF before the chunk" drop are not in KINDS: no natural input of
these classes reaches them with margin (test_branches_no_case_reaches records that none does).
"""
import collections

import numpy as np
import pytest

import oracle_py as O
import phy_fixtures as F
import sync_edge_cases as E

IDS = [c.id for c in E.CASES]


def _rates(c):
    _, (_, _, _, _, L, M) = F.case(c.name)
    return L, M


def _key(reports):
    return [(r["det_time"], r["N_eff_TX"], r["fine_64"]) for r in reports]


# ---------------------------------------------------------------- 1. the branch every kind is there for
def _reaches(c):
    """the predicate of c.kind on the oracle's reports and trace"""
    reps, tr = E.oracle(c)
    g, (L, M) = E.geometry(c), _rates(c)
    hw = lambda dect: dect * L / M
    n_ant = F.case(c.name)[1][2]
    start = c.starts[0]
    k = c.kind
    if k == "head_none":  # the STF ends before anything may be detected, or its coarse peak is dropped
        return len(reps) == 0 and tr["ignored_steps"] > 0 and (start + hw(g["stf_len"]) <= hw(g["stf_len"] + g["pattern"])
                                                               or tr["stf_before_chunk"] > 0)
    if k == "head_found":  # found although (part of) its STF lies in the ignored head
        return _key(reps)[0][2] == start and len(reps) == 1 and start < 2 * hw(g["stf_len"] + g["pattern"])
    if k == "tail_found":  # detected within the last 2.5 STF of the search
        return len(reps) == 1 and reps[0]["fine_64"] == start and reps[0]["det_time"] > g["search_len"] - 5 * g["stf_len"] // 2
    if k == "tail_none":  # the search ends before the STF can be detected
        return len(reps) == 0 and start < c.S_win - hw(g["stf_len"]) and start > hw(g["search_len"] - g["stf_len"])
    if k == "cut_steps":
        return tr["resampler_outside"] > 0 and c.S_win < hw(g["search_len"]) and len(reps) == 1 and tr["fine_outside"] == 0
    if k == "cut_fine":
        return len(reps) == 1 and tr["fine_outside"] > 0 and c.S_win >= start + hw(g["stf_len"])
    if k == "cut_coarse":  # the coarse search range [det_time_jb, det_time_jb + D) ends past the window
        full = O.sync(E.sync_cfg(c), E.uncut(c), max_reports=1)
        return len(full) == 1 and c.S_win < hw(full[0]["det_time_jb"] + g["D"]) and c.S_win > start + hw(g["stf_len"]) * 3 // 4
    if k == "cut_stf":
        return start + hw(g["stf_len"]) // 4 < c.S_win < start + hw(g["stf_len"]) * 3 // 4 and tr["resampler_outside"] > 0
    if k in ("gate_rms_min", "gate_rms_max", "gate_zero"):
        a = [i for i, x in enumerate(c.gains) if x != 1.0][0]
        cnt = tr["rms_max_rej" if k == "gate_rms_max" else "rms_min_rej"][a]
        return len(reps) == 1 and cnt > 0 and tr["invalid_at_peak"][a] == (1 if k == "gate_zero" else 0) and \
            (a != 0 or reps[0]["det_ant"] != 0)
    if k == "gate_one_live":
        return len(reps) == 1 and reps[0]["det_ant"] == 3 and tr["rms_min_rej"][0] > 0 and tr["rms_min_rej"][1] > 0 and \
            tr["rms_max_rej"][2] > 0 and tr["invalid_at_peak"][0] == 1
    if k == "gate_n_lim":
        return _key(reps) == [(reps[0]["det_time"], E.n_eff_tx(c), start)] and n_ant == 4 and c.n_lim == 2
    if k == "b2b_gap":  # both found: the second STF lies behind the first report's skip_after_peak
        return [r["fine_64"] for r in reps] == list(c.starts)
    if k == "b2b_overlap":
        return len(reps) >= 1 and reps[0]["fine_64"] == c.starts[0]
    raise AssertionError(k)


@pytest.mark.parametrize("cid", IDS)
def test_case_reaches_its_branch(cid):
    c = E.BY_ID[cid]
    reps, tr = E.oracle(c)
    assert _reaches(c), (cid, c.kind, _key(reps), {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in tr.items()})
    for r in reps:  # wherever the oracle reports, it reports a transmitted packet
        assert r["fine_64"] in c.starts and r["N_eff_TX"] == E.n_eff_tx(c), (cid, r["fine_64"], c.starts)


KINDS = ["b2b_gap", "b2b_overlap", "cut_coarse", "cut_fine", "cut_steps", "cut_stf", "gate_n_lim", "gate_one_live",
         "gate_rms_max", "gate_rms_min", "gate_zero", "head_found", "head_none", "tail_found", "tail_none"]


def test_kinds_reached_are_the_literal_list():
    assert sorted({c.kind for c in E.CASES if _reaches(c)}) == KINDS


def test_branches_no_case_reaches():
    """nvalid == 0 (false alarm) and wpk < stf_len - 1 (STF before the chunk) are reached by none of these inputs
    and stay untested rather than built artificially. The second needs a detection at the first evaluated step
    (det_time = stf_len + pattern) whose peak lies in the first few positions of its coarse range, i.e. a packet
    that starts within ~2 samples of the window start and is still detected one pattern after its STF ended: at
    starts 0 .. 4 the oracle reports nothing, or something that another seed does not (see the margin rule)."""
    assert all(E.oracle(c)[1]["false_alarms"] == 0 and E.oracle(c)[1]["stf_before_chunk"] == 0 for c in E.CASES)


# ---------------------------------------------------------------- 2. margin
def _margin(c):
    """None, or why the case may not stay"""
    win = E.searched(c, E.window(c)[0])
    reps, tr = E.oracle(c)
    flo = O.sync(E.sync_cfg(c), win, max_reports=c.max_reports, use_float=True)
    if _key(flo) != _key(reps):
        return "float path %s, double path %s" % (_key(flo), _key(reps))
    other = O.sync(E.sync_cfg(c), E.searched(c, E.second_seed(c)), max_reports=c.max_reports)
    if len(other) != len(reps):
        return "second seed reports %d, first %d" % (len(other), len(reps))
    if not reps and tr["closest_metric"] < 0.1:
        return "a step's metric within %.3f of the threshold" % tr["closest_metric"]
    return None


@pytest.mark.parametrize("cid", IDS)
def test_margin(cid):
    assert _margin(E.BY_ID[cid]) is None, cid


def test_minimum_kept():
    n = collections.Counter((c.cls, c.kind, c.name) for c in E.CASES)
    for kind in ("head_none", "head_found", "tail_found", "tail_none"):  # both outcomes on each side
        assert n[("position", kind, "C2")] >= 1, kind
    assert n[("position", "head_none", "C2")] + n[("position", "head_found", "C2")] >= 6
    assert n[("position", "tail_none", "C2")] + n[("position", "tail_found", "C2")] >= 6
    for name in ("C3", "os2_u2b2_tm1"):
        assert sum(v for (cls, kind, nm), v in n.items() if nm == name and kind.startswith("head")) >= 3
        assert sum(v for (cls, kind, nm), v in n.items() if nm == name and kind.startswith("tail")) >= 3
    for name in ("C2", "C3", "lm1_1_u8b16", "lm40_27_u8b12_tm5", "os2_u2b2_tm1"):  # each cut, even and odd, per form
        for kind in ("cut_steps", "cut_fine", "cut_coarse", "cut_stf"):
            sizes = [c.S_win for c in E.TRUNCATION if c.name == name and c.kind == kind]
            assert any(s % 2 for s in sizes) and any(s % 2 == 0 for s in sizes), (name, kind, sizes)
    assert any(c.snr_db is None for c in E.TRUNCATION)
    assert set(E.FORMS["C3"][i].get(k) for i, k in ((1, "DNRP_SYNC_PIPE"), (2, "DNRP_SYNC_STREAM"))) == {"0"}
    assert {f.get("DNRP_SYNC_ROUNDS") for f in E.FORMS["C3"]} >= {"0", "2"}
    for name in ("tm1_txdiv2", "mrc4_16qam"):  # all three states of antenna 0 at both antenna counts
        for kind in ("gate_rms_min", "gate_rms_max", "gate_zero"):
            assert any(c.name == name and c.kind == kind and c.gains[0] != 1.0 for c in E.GATES), (name, kind)
    assert len(E.LAYOUTS) == 4 and len(E.STREAM_STARTS) >= 12 and E.STREAM_BOUNDARY in E.STREAM_STARTS
    assert n[("backtoback", "b2b_gap", "C2")] >= 3 and n[("backtoback", "b2b_overlap", "C2")] == 1


def test_geometry_table():
    """the sizes the module's table states"""
    want = {"C2": (4, 124, 142, 897), "C3": (64, 2560, 2844, 14330), "lm1_1_u8b16": (64, 2304, 2560, 13312),
            "lm40_27_u8b12_tm5": (48, 2560, 2844, 14320), "os2_u2b2_tm1": (16, 640, 711, 3760),
            "tm1_txdiv2": (32, 1280, 1422, 7680), "mrc4_16qam": (16, 640, 711, 3760)}
    for name, (S, chunk) in E.SIZES.items():
        c = E.Case("g", "", "", name, S, S, chunk, (), 0, None, None, None, None, 1)
        g, (L, M) = E.geometry(c), _rates(c)
        got = (g["step"], g["stf_len"] * L // M, (g["stf_len"] + g["pattern"]) * L // M, g["search_len"] * L // M)
        assert got == want[name], (name, got)


# ---------------------------------------------------------------- stream sweep
@pytest.mark.parametrize("start", E.STREAM_STARTS)
def test_stream_position(start):
    """the packet is found exactly once at its true time, by the double and the float path and from another seed"""
    ring, g0 = E.stream_ring(start)
    ref, dup = E.stream_oracle(ring, g0)
    assert [t - g0 for t, _, _ in ref] == [start], (start, [t - g0 for t, _, _ in ref])
    flo, dup_f = E.stream_oracle(ring, g0, use_float=True)
    assert [(t, k) for t, k, _ in flo] == [(t, k) for t, k, _ in ref] and dup_f == dup
    ring2, g2 = E.stream_ring(start, seed=1600 + start)
    assert [t - g2 for t, _, _ in E.stream_oracle(ring2, g2)[0]] == [start]


def test_stream_sweep_crosses_the_finders():
    """over the sweep the first finding chunk moves from k to k + 1; the search overlaps the next chunk by 4 STF
    (498 samples > chunk 400), so every position is found again by a later chunk and dropped by the baton, next
    to the hand-over by two later chunks"""
    first, dups = [], []
    for start in E.STREAM_STARTS:
        ring, g0 = E.stream_ring(start)
        ref, dup = E.stream_oracle(ring, g0)
        first.append(ref[0][1])
        dups.append(dup)
    print("finding chunk per start", first, "double detections", dups)
    assert len(set(first)) >= 2 and first == sorted(first)
    assert set(dups) == {1, 2}


# ---------------------------------------------------------------- 3. wrong-kernel proofs
def test_wrong_kernel_reads_past_the_window():
    """truncation: the oracle on the uncut samples (a kernel without the zeros outside [0, S_win)) reports
    something else on a cut of every kind but cut_steps, whose tail holds no second packet"""
    changed = collections.Counter()
    for c in E.TRUNCATION:
        full = O.sync(E.sync_cfg(c), E.uncut(c), max_reports=c.max_reports)
        reps = E.oracle(c)[0]
        same = _key(full) == _key(reps) and all(
            abs(a["cfo_frac"] - b["cfo_frac"]) < 2e-6 and np.allclose(a["xc_metric"], b["xc_metric"], rtol=1e-3) and
            np.allclose(a["coarse_metric"], b["coarse_metric"], rtol=1e-3, atol=1e-6) for a, b in zip(full, reps))
        changed[c.kind] += not same
    print("cuts whose report a read past S_win changes beyond the GPU gates:", dict(changed))
    assert changed["cut_fine"] > 0 and changed["cut_coarse"] > 0 and changed["cut_stf"] > 0


def test_wrong_kernel_ignores_the_rms_gates():
    """gates: with antenna 0 not gated the detection antenna is 0 again"""
    n = 0
    for c in E.GATES:
        if c.gains is None or c.gains[0] in (1.0, 0.0):  # a silent antenna detects nothing, gated or not
            continue
        reps = E.oracle(c)[0]
        bad = O.sync_trace(E.sync_cfg(c), E.window(c)[0], max_reports=c.max_reports, mutant=O.SYNC_MUTANT_ANT0_UNGATED)[0]
        assert reps[0]["det_ant"] != 0 and bad and bad[0]["det_ant"] == 0, (c.id, reps[0]["det_ant"], bad)
        n += 1
    assert n >= 4


def test_wrong_kernel_searches_every_antenna():
    """N_ant_limited: a search of all four antennas reports the hidden packet first"""
    c = E.BY_ID["gate_n_lim_2_of_4"]
    all4 = O.sync(E.sync_cfg(c._replace(n_lim=None)), E.window(c)[0], max_reports=c.max_reports)
    assert all4[0]["fine_64"] == c.hidden[0] and E.oracle(c)[0][0]["fine_64"] == c.starts[0]


def test_wrong_kernel_position():
    """position: a search that starts one STF earlier / runs one chunk longer (the window moved, the chunk grown)
    reports the packets the head and the tail cases must not"""
    for c in E.POSITION:
        if c.name != "C2" or c.kind not in ("head_none", "tail_none"):
            continue
        win = E.window(c)[0]
        if c.kind == "head_none":
            moved = np.concatenate([win[:, -200:], win[:, :-200]], axis=1)  # 200 samples of the noise tail in front
            got = O.sync(E.sync_cfg(c), moved, max_reports=1)
            assert [r["fine_64"] for r in got] == [c.starts[0] + 200], c.id
        else:
            got = O.sync(E.sync_cfg(c, chunk=c.chunk + 400), win, max_reports=1)
            assert [r["fine_64"] for r in got] == [c.starts[0]], c.id


def test_wrong_kernel_skips_skip_after_peak():
    """back to back: the first packet alone (the second removed) gives one report, so the second report of each
    pair is the second STF and not a second detection of the first packet"""
    for c in E.BACKTOBACK:
        reps = E.oracle(c)[0]
        alone = O.sync(E.sync_cfg(c), E._build(c._replace(starts=c.starts[:1]), c.seed)[0], max_reports=c.max_reports)
        assert [r["fine_64"] for r in alone] == [c.starts[0]], c.id
        if c.kind == "b2b_gap":
            assert len(reps) == 2
