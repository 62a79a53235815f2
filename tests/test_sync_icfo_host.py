"""Integer CFO search of the synchronisation, host side (no GPU): the cell set of a candidate
(dnrp_query_table "sync_icfo_cells") against the oracle's STF, the argument checks that need no context, and the
margin proof of the inputs tests/test_gpu_sync_icfo.py uses: the estimator restated in numpy
(tests/sync_icfo_cases.py) returns the injected k on every L = M = 1 window at the oracle's coarse peak and
fractional CFO, the runner-up at most 0.95 of the winner.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O
import sync_beta_cases as K
import sync_icfo_cases as I

dnrp = pytest.importorskip("dnrp")

EINVAL = -1


def test_setter_getter_null_context():
    L = dnrp.lib()
    r = C.c_uint32(7)
    for v in (0, 1, 4, 5):
        assert L.dnrp_ctx_set_sync_icfo_search(None, v) == EINVAL, v
    assert L.dnrp_ctx_get_sync_icfo_search(None, C.byref(r)) == EINVAL
    assert r.value == 7  # nothing written on an error
    s, k = np.zeros((1, 8, 9), np.float32), np.zeros(1, np.int32)
    assert L.dnrp_rx_sync_icfo_scores(None, 1, C.c_void_p(s.ctypes.data), C.c_void_p(k.ctypes.data), None) == EINVAL
    for name in ("set_sync_icfo_search", "sync_icfo_search", "sync_icfo_scores"):
        assert hasattr(dnrp.Phy, name), name


@pytest.mark.parametrize("n_eff", [1, 2, 4])
@pytest.mark.parametrize("N,b", [(128, 1), (64, 1), (128, 2), (256, 2), (512, 1), (512, 4), (512, 8), (768, 12),
                                 (2048, 16)])
def test_cells_are_the_stf_cells_shifted(N, b, n_eff):
    """candidate k sums the occupied STF subcarriers of b (the same set for every N_eff_TX: the sequence is rotated
    over the cells, the cells stay) moved by 4 k bins, mod N; nothing where the moved set would reach N / 2"""
    stf = O.stf(b, n_eff)
    sub = np.nonzero(stf)[0] - 28 * b
    assert len(sub) == 14 * b and sub.min() == -28 * b and sub.max() == 28 * b
    for k in range(-I.MAX_RANGE, I.MAX_RANGE + 1):
        got = dnrp.sync_icfo_cells(N, b, k)
        if 4 * (7 * b + abs(k)) >= N // 2:
            assert len(got) == 0, (k, got)
        else:
            assert np.array_equal(np.sort(got), np.sort((sub + 4 * k) % N)), k
            assert len(set(got.tolist())) == len(got)


def test_cells_argument_errors():
    L = dnrp.lib()

    def n(*a):
        arr = np.asarray([v & 0xFFFFFFFF for v in a], np.uint32)
        return L.dnrp_query_table(b"sync_icfo_cells", C.c_void_p(arr.ctypes.data), len(arr), None, 0)

    assert n(128, 1, -2) == 14 and n(64, 1, 0) == 14 and n(64, 1, 1) == 0 and n(64, 1, -1) == 0  # |k| < b at os_min 1
    assert n(128, 2, 1) == 28 and n(128, 2, 2) == 0  # 4 (14 + 2) = 64 = N / 2: the example of a clipped range
    assert n(128, 3, 0) == EINVAL    # b not in b_idx2b
    assert n(100, 1, 0) == EINVAL    # N no multiple of 64
    assert n(64, 2, 0) == EINVAL and n(0, 1, 0) == EINVAL  # N = 64 b_max os_min is at least 64 b
    assert n(128, 1, 5) == EINVAL and n(128, 1, -5) == EINVAL
    assert n(128, 1) == EINVAL       # argument count


@pytest.mark.parametrize("q", I.HOST_CASES, ids=lambda q: q.id)
def test_inputs_have_margin(q):
    """A condition on the inputs of tests/test_gpu_sync_icfo.py, not a measurement of the library: on every window
    the oracle search of the packet's class still detects the shifted packet and reports f, and the estimator in
    double, at that coarse peak and fractional CFO and with the packet's b, returns the injected k with the
    runner-up's summed score at most 0.95 of the winner's (noise-free it loses two of the 14 b cells: 0.857 at
    b = 1, 0.929 at b = 2). Measured: 0.856-0.859 at b = 1, 0.925-0.931 at b = 2."""
    u, b_max, os_min, _, _, _, _, b = q.c
    osc = K.oracle_sync_cfg(q.c)
    for k, win, start, _ in I.all_windows(q):
        o = O.sync(osc, win, max_reports=1)
        assert len(o) == 1 and abs(o[0]["coarse_local"] - start) <= 3, (k, o)
        sc = I.scores(win, u, q.N, b, o[0]["coarse_local"], o[0]["cfo_frac"], q.rng)
        for kk in range(-I.MAX_RANGE, I.MAX_RANGE + 1):
            on = abs(kk) <= q.rng and I.searched(q.N, b, kk)
            assert np.all((sc[:, kk + I.MAX_RANGE] >= 0) if on else (sc[:, kk + I.MAX_RANGE] == -1)), kk
        k_hat, s = I.decide(sc)
        assert k_hat == k, (k, k_hat, s)
        live = np.sort(s[s >= 0])[::-1]
        if len(live) > 1:
            print(q.id, "k", k, "runner-up / winner", live[1] / live[0])
            assert live[1] <= 0.95 * live[0], (k, s)
        else:
            assert k == 0 and len(live) <= 1


@pytest.mark.parametrize("q", [q for q in I.HOST_CASES if q.beta], ids=lambda q: q.id)
def test_beta_inputs_within_two_cells_keep_their_b(q):
    """the other condition of the cases that run with the beta search on: the beta restatement
    (sync_beta_cases.estimate_beta) returns the packet's b on the shifted window for |k| <= 2. Beyond that the
    shifted packet's power crosses a band edge: printed, not asserted -- there the second beta
    pass decides, whose condition is asserted for every k: on the window with 4 k subcarriers taken out the
    restatement returns b, and with the first decision's b (right or not) the estimator still returns k."""
    u, b_max, os_min, _, _, _, _, b = q.c
    osc = K.oracle_sync_cfg(q.c)
    for k, win, _, _ in I.all_windows(q):
        at = O.sync(osc, win, max_reports=1)[0]["coarse_local"]
        b_est, ratios = K.estimate_beta(win, u, b_max, os_min, at, 10 ** (-10 / 20))
        print(q.id, "k", k, "b_est", b_est, "ratios", ratios)
        if abs(k) <= 2:
            assert b_est == b, (k, b_est, ratios)
        b_rot, r_rot = K.estimate_beta(I.derotate(win, k, q.N), u, b_max, os_min, at, 10 ** (-10 / 20))
        assert b_rot == b and all(r <= 0.1 or r >= 0.45 for r in r_rot), (k, b_rot, r_rot)
        o = O.sync(osc, win, max_reports=1)[0]
        assert I.decide(I.scores(win, u, q.N, b_est, at, o["cfo_frac"], q.rng))[0] == k, (k, b_est)
