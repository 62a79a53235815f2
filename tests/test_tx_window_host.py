"""TX OFDM windowing, host side (no GPU): dnrp_tx_window -- the raised-cosine table the device uses --
against the reference's own raised_cosine_window_rising_edge (tests/golden/ref_tx_window.json, recorded
from the compiled reference), the window length rule of dft/windowing.cpp:34-39 at its rounding
edges, and the argument checks of dnrp_tx_window and dnrp_ctx_set_tx_windowing."""
import ctypes as C
import json
import os

import numpy as np
import pytest

dnrp = pytest.importorskip("dnrp")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_tx_window.json")
EINVAL = -1

# (N_b_DFT_os, fraction) -> N = roundf(N_b_DFT_os / 8 * fraction), one pair for every N of the fixture
PAIRS = [(64, 0.25, 2), (64, 0.4, 3), (128, 0.25, 4), (128, 0.3, 5), (256, 0.25, 8), (512, 0.25, 16),
         (1024, 0.25, 32), (1024, 1.0, 128), (8192, 0.25, 256)]


def _golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert "raised_cosine.cpp" in g["generated_by"]
    return {int(k): np.array(v, np.uint32).view(np.float32) for k, v in g["rising_edge"].items()}


def test_fixture_covers_every_pair():
    assert sorted(_golden()) == sorted(n for _, _, n in PAIRS) == [2, 3, 4, 5, 8, 16, 32, 128, 256]


@pytest.mark.parametrize("nd,fraction,n", PAIRS)
def test_window_matches_reference(nd, fraction, n):
    ref = _golden()[n]
    got = dnrp.tx_window(nd, fraction)
    assert got.dtype == np.float32 and got.shape == (n,) == ref.shape
    # within one float ulp of the reference's value (libm builds may differ in cosf)
    ulp = np.spacing(np.abs(ref))
    assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= ulp), (got, ref)
    # the shape of a rising edge: from (nearly) 0 up to below 1, the midpoint at 1/2 for even N
    assert got[0] < 1e-12 and np.all(np.diff(got) > 0) and got[-1] < 1.0
    if n % 2 == 0:
        assert abs(got[n // 2] - 0.5) < 1e-6


@pytest.mark.parametrize("nd,fraction,want", [(64, 0.3, 2), (128, 0.3, 5), (1024, 1.0, 128), (64, 0.1, EINVAL),
                                              (64, 0.25, 2), (64, 0.18, EINVAL), (64, 0.19, 2), (4096, 0.25, 128)])
def test_window_length_rule(nd, fraction, want):
    """N = (uint32_t)roundf(float(N_b_DFT_os / 8) * fraction), N >= 2 (8 * 0.3 = 2.4 -> 2, 16 * 0.3 = 4.8 -> 5,
    8 * 0.1 = 0.8 -> 1: refused, 8 * 0.18 = 1.44 -> 1: refused, 8 * 0.19 = 1.52 -> 2)."""
    assert dnrp.lib().dnrp_tx_window(nd, fraction, None, 0) == want
    if want == EINVAL:
        with pytest.raises(dnrp.DnrpError) as e:
            dnrp.tx_window(nd, fraction)
        assert e.value.code == EINVAL
    else:
        assert len(dnrp.tx_window(nd, fraction)) == want


def test_tx_window_argument_errors():
    L = dnrp.lib()
    buf = np.full(8, 7.0, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    assert L.dnrp_tx_window(100, 0.25, None, 0) == EINVAL          # N_b_DFT_os % 8 != 0
    assert L.dnrp_tx_window(0, 0.25, None, 0) == EINVAL
    for bad in (0.0, -0.25, 1.0000001, float("inf"), float("-inf"), float("nan")):
        assert L.dnrp_tx_window(128, bad, None, 0) == EINVAL, bad  # fraction outside (0, 1]
    assert L.dnrp_tx_window(64, 0.1, p, 8) == EINVAL               # N < 2
    assert L.dnrp_tx_window(128, 0.25, p, 3) == EINVAL             # cap < N = 4
    assert np.all(buf == 7.0)                                      # nothing written on an error
    assert L.dnrp_tx_window(128, 0.25, p, 4) == 4
    assert np.all(buf[:4] == dnrp.tx_window(128, 0.25)) and np.all(buf[4:] == 7.0)


def test_set_tx_windowing_null_context():
    L = dnrp.lib()
    for f in (0.0, 0.25, 2.0, float("nan")):
        assert L.dnrp_ctx_set_tx_windowing(None, f) == EINVAL
