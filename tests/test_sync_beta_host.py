"""Beta search of the synchronisation, host side (no GPU): the argument checks of
dnrp_ctx_set_sync_beta_search / dnrp_ctx_get_sync_beta_search that need no context (the round trip runs
on a context in tests/test_gpu_sync_beta.py: a context opens the device), the per-b STF templates
(dnrp_query_table "sync_template") against the oracle's stf_template, and the margin proof of the inputs
the GPU file uses: the estimator restated in numpy (tests/sync_beta_cases.py) returns the transmitted b
on every L = M = 1 window, with every ratio it forms far from the threshold.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O
import sync_beta_cases as K

dnrp = pytest.importorskip("dnrp")

EINVAL = -1
LM = [(1, 1), (10, 9), (40, 27)]


def _tmpl(u, b_max, os_min, L, M, b, n_eff):
    return dnrp.query_table("sync_template", u, b_max, os_min, L, M, b, n_eff).view(np.complex64)


def _peak_ulps(got, ref):
    """largest component difference in float32 ulps of the template's peak magnitude"""
    ulp = float(np.spacing(np.float32(np.abs(ref).max())))
    d = got.astype(np.complex128) - ref.astype(np.complex128)
    return max(np.abs(d.real).max(), np.abs(d.imag).max()) / ulp


def test_setter_getter_null_context():
    L = dnrp.lib()
    on, db, lin = C.c_uint32(7), C.c_float(7.0), C.c_float(7.0)
    for args in ((0, -10.0), (1, -10.0), (2, -10.0), (1, float("nan")), (1, float("inf"))):
        assert L.dnrp_ctx_set_sync_beta_search(None, *args) == EINVAL, args
    assert L.dnrp_ctx_get_sync_beta_search(None, C.byref(on), C.byref(db), C.byref(lin)) == EINVAL
    assert (on.value, db.value, lin.value) == (7, 7.0, 7.0)  # nothing written on an error
    assert hasattr(dnrp.Phy, "set_sync_beta_search") and hasattr(dnrp.Phy, "sync_beta_search")


@pytest.mark.parametrize("L,M", LM)
@pytest.mark.parametrize("u,b_max,os_min", [(1, 4, 1), (2, 8, 1), (1, 12, 1), (1, 2, 2)])
def test_template_b_max_row_is_the_oracle_template(u, b_max, os_min, L, M):
    """b = b_max: the template the fine search had before (the existing code path). Both sides compute in
    double and round once to float, so a value can differ by one rounding step of its own size, which is
    at most one float32 ulp of the peak. Measured here: 0 to 1.7e-9 peak ulps (single rounding flips on
    samples of small magnitude)."""
    scfg = O.sync_cfg(u, b_max, os_min, L, M)
    for n_eff in (1, 2, 4, 8):
        got, ref = _tmpl(u, b_max, os_min, L, M, b_max, n_eff), O.stf_template(scfg, n_eff)
        assert got.shape == ref.shape == (O.sync_geometry(scfg)["tmpl_len"],)
        d = _peak_ulps(got, ref)
        print("b_max row", (u, b_max, os_min, L, M, n_eff), "peak ulps", d)
        assert d <= 1.0, (n_eff, d)


@pytest.mark.parametrize("u,b_max,os_min", [(1, 4, 1), (2, 8, 1), (1, 2, 2), (1, 16, 1)])
def test_template_rows_below_b_max(u, b_max, os_min):
    """b < b_max at L = M = 1, b_max / b an integer: the row is the oracle's template of the class (u, b) at
    os_min b_max / b (same N_b_DFT_os, same cover pattern length, the STF and scale of b). Bound: twice the
    b = b_max rows' (measured 0..1.7e-9, bounded by one rounding step = 1 peak ulp there): 2 float32 ulps
    of the peak magnitude. Measured on these rows: 0 to 1.7e-9."""
    for b in K.B_IDX2B:
        if b >= b_max or b_max % b:
            continue
        for n_eff in (1, 2, 4, 8):
            got = _tmpl(u, b_max, os_min, 1, 1, b, n_eff)
            ref = O.stf_template(O.sync_cfg(u, b, os_min * b_max // b, 1, 1), n_eff)
            assert got.shape == ref.shape
            d = _peak_ulps(got, ref)
            print("row", (u, b_max, os_min, b, n_eff), "peak ulps", d)
            assert d <= 2.0, (b, n_eff, d)


def _tx_half_length_hw(os_min, L, M):
    """half length of the TX resampling filter in hw samples (kaiser design at the L-fold rate)"""
    q = lambda k: O.query_param("resampler_param_t::%s" % k)
    key = "[0][%d]" % os_min
    h = O.kaiser(q("f_pass_norm" + key) / L, q("f_stop_norm" + key) / L, q("PASSBAND_RIPPLE_DONT_CARE"),
                 q("f_stop_att_dB" + key))
    return -(-(len(h) // 2 + 1) // M)


def _rho(a, b):
    a, b = a.astype(np.complex128), b.astype(np.complex128)
    return abs(np.vdot(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b))


@pytest.mark.parametrize("u,b_max,os_min,bs", [(1, 4, 1, (1, 2)), (2, 8, 1, (2, 4)), (1, 12, 1, (8,))])
def test_template_rows_at_10_9_match_the_transmitted_stf(u, b_max, os_min, bs):
    """10/9, b < b_max (no oracle template: it would take the filters of a larger os_min): the interior of
    the row (without the TX filter's half length at either end, where the template's flush differs from a
    packet that goes on) against the first tmpl_len samples of antenna 0 of an oracle TM0 packet of that b,
    CFO 0. Its defect 1 - rho may be at most twice the b = b_max row's against its own packet, measured in
    the same test. Both measure 2e-16 to 2e-15 here: the two float vectors agree so closely that 1 - rho
    sits at the rounding floor of rho's own double sums, so the bound adds that floor, n 2^-53 for the n
    summed terms (the worst-case summation error of a dot product), 5e-14 to 2e-13 -- a template with a
    wrong offset, scale pattern or cover pattern has a defect above 1e-2."""
    L, M = 10, 9
    cut = _tx_half_length_hw(os_min, L, M)
    rng = np.random.default_rng(5)

    def defect(b):
        t = _tmpl(u, b_max, os_min, L, M, b, 1)
        y, _ = K.packet(rng, (u, b_max, os_min, L, M, 1, 0, b), 0.0)
        assert len(t) > 4 * cut
        return 1.0 - _rho(t[cut:len(t) - cut], y[0, cut:len(t) - cut]), (len(t) - 2 * cut) * 2.0 ** -53

    d_max, floor = defect(b_max)
    assert d_max < 1e-6  # the existing row against its own packet: float rounding only
    for b in bs:
        d, _ = defect(b)
        print("10/9 row", (u, b_max, os_min, b), "defect", d, "b_max row", d_max, "floor", floor)
        assert d <= 2.0 * d_max + floor, (b, d, d_max)


def test_template_argument_errors():
    L = dnrp.lib()

    def n(*a):
        arr = np.asarray(a, np.uint32)
        return L.dnrp_query_table(b"sync_template", C.c_void_p(arr.ctypes.data), len(arr), None, 0)

    assert n(1, 4, 1, 10, 9, 2, 1) == 2 * O.sync_geometry(O.sync_cfg(1, 4, 1, 10, 9))["tmpl_len"]
    assert n(1, 4, 1, 10, 9, 8, 1) == EINVAL    # b > b_max
    assert n(1, 4, 1, 10, 9, 3, 1) == EINVAL    # b not in b_idx2b
    assert n(1, 16, 1, 10, 9, 10, 1) == EINVAL
    for bad in (0, 3, 5, 16):
        assert n(1, 4, 1, 10, 9, 2, bad) == EINVAL, bad  # N_eff_TX outside {1, 2, 4, 8}
    assert n(3, 4, 1, 10, 9, 2, 1) == EINVAL    # u
    assert n(1, 4, 1, 10, 9, 2) == EINVAL       # argument count


MARGIN_CASES = [c for c in K.PARITY + K.TRUTH if c[3] == c[4] == 1]


def _margin(win, u, b_max, os_min, at, b):
    thr = 10 ** (-10 / 20)
    for d in (0, -1, 1, -8 * b_max * os_min, 8 * b_max * os_min):
        b_est, ratios = K.estimate_beta(win, u, b_max, os_min, at + d, thr)
        assert b_est == b, (d, b_est, ratios)
        assert all(r <= 0.1 or r >= 0.45 for r in ratios), (d, ratios)


@pytest.mark.parametrize("seed,cases", [(77, K.MIXED_WINDOW), (78, K.MIXED_RING)])
def test_mixed_inputs_have_margin(seed, cases):
    """the same condition on the two-packet windows (one window, and the stream in the ring): at the coarse
    peak of packet k as the oracle search of that packet's b finds it (its k-th report, fine peak exact)"""
    win, starts = K.two_packet_window(seed, *cases)
    for k, c in enumerate(cases):
        u, b_max, os_min, _, _, n_ant, _, b = c
        osc = O.sync_cfg(u, b, os_min=os_min * b_max // b, L=1, M=1, n_ant=n_ant, chunk_len=win.shape[1] * 7 // 8)
        ref = O.sync(osc, win, max_reports=2)
        assert len(ref) == 2 and ref[k]["fine_64"] == starts[k]
        _margin(win, u, b_max, os_min, ref[k]["coarse_local"], b)


@pytest.mark.parametrize("c", MARGIN_CASES, ids=K.case_id)
def test_inputs_have_margin(c):
    """A condition on the inputs of tests/test_gpu_sync_beta.py, not a measurement of the library: on every
    L = M = 1 window the estimator in double returns the transmitted b at the oracle's coarse peak, one
    sample either side of it and half a pattern (8 b_max os_min samples) either side, and every ratio it
    forms is <= 0.1 or >= 0.45 (threshold 10^(-10/20) = 0.316)."""
    u, b_max, os_min, _, _, _, _, b = c
    for win, start, _, _ in K.windows(c):
        if b_max % b == 0:
            o = O.sync(K.oracle_sync_cfg(c), win, max_reports=1)
            assert len(o) == 1 and o[0]["fine_64"] == start
            at = o[0]["coarse_local"]
        else:  # no oracle search for this ratio: the transmitted start
            at = start
        _margin(win, u, b_max, os_min, at, b)
