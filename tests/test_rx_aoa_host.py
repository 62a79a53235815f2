"""Angle-of-arrival report on a machine without a GPU (dnrp_aoa_estimate, the host twin of rx_aoa_kernel's scan;
tests/aoa_cases.py holds the cases, the numpy restatement and the pilot model).

1. The twin equals the restatement on random Hermitian PSD R and on exact a a^H for the three geometries:
   grid_idx exact; az_rad, peak and the spectrum within 1e-9 (both double on the same float R, both rounded to
   float once at the end).
2. Interpolation bias of the restatement on exact a a^H: 181 points over +-90 deg, |az| <= 75 deg, line arrays of 2, 4
   and 8: <= 0.05 deg (measured 0.0325 deg; 0.121 deg at 91 points, 0.0081 deg at 361: it falls with the square of
   the step). The 360-point cyclic scan on the 8-antenna circle: <= 0.001 deg (measured 0.0002 deg).
3. The noisy L = M = 1 cases at 10 dB: the pilot model's own azimuth stays within twice the recorded error of the
   truth (aoa_cases.NOISY_ERR_DEG), so the inputs are decidable from the CPU alone.
4. A model that conjugates the steering vector, or swaps two antennas, misses item 3's bound.
5. DNRP_EINVAL: a NULL context, and dnrp_aoa_estimate's refusals.
"""
import ctypes as C

import numpy as np
import pytest

import aoa_cases as AC

dnrp = pytest.importorskip("dnrp")

EINVAL = -1
GEOMETRIES = {"ula2": (AC.ula(2), AC.SCAN_ULA), "ula4": (AC.ula(4), AC.SCAN_ULA), "uca8": (AC.uca(8), AC.SCAN_UCA)}


def _same(pos, scan, R):
    n = len(pos)
    ref = AC.estimate(pos, *scan, R)
    got = dnrp.aoa_estimate(pos, *scan, R)
    assert got["grid_idx"] == ref["grid_idx"]
    assert abs(got["az_rad"] - float(ref["az32"])) <= 1e-9, (got["az_rad"], ref["az_rad"])
    assert abs(got["peak"] - float(ref["peak32"])) <= 1e-9, (got["peak"], ref["peak"])
    assert np.max(np.abs(got["spectrum"].astype(np.float64) - ref["spectrum"].astype(np.float32))) <= 1e-9
    R32 = np.asarray(R)[:n, :n].astype(np.complex64)
    lag = complex(np.sum(np.diag(R32, -1).astype(np.complex128)))
    assert abs(got["lag"] - complex(np.complex64(lag))) <= 1e-9 * max(1.0, abs(lag))
    return got


# ---------------------------------------------------------------- 1. twin against numpy
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_twin_equals_restatement(name):
    pos, scan = GEOMETRIES[name]
    n = len(pos)
    rng = np.random.default_rng(5)
    for _ in range(20):  # random Hermitian PSD
        X = rng.standard_normal((n, n + 2)) + 1j * rng.standard_normal((n, n + 2))
        _same(pos, scan, (X @ X.conj().T) * 10.0 ** rng.uniform(-6, 3))
    lo, hi, _ = scan
    for az in rng.uniform(lo, hi, 40):  # exact a a^H
        a = AC.steering(pos, az)
        got = _same(pos, scan, np.outer(a, a.conj()))
        assert got["peak"] >= 1.0 - 1e-3
    got = dnrp.aoa_estimate(pos, *scan, np.zeros((n, n)))  # tr R = 0
    assert (got["grid_idx"], got["az_rad"], got["peak"]) == (AC.NONE, 0.0, 0.0) and not np.any(got["spectrum"])


def test_first_maximum_wins():
    # the two-antenna half-wavelength line has equal maxima at -90 and +90 deg for a source at either end
    pos, scan = AC.ula(2), AC.SCAN_ULA
    R = np.array([[1, -1], [-1, 1]], np.complex64)  # a(+-90 deg) = (1, -1)
    got = _same(pos, scan, R)
    assert got["grid_idx"] in (0, AC.SCAN_ULA[2] - 1)
    # a spectrum falling from the first grid point on: index 0, no interpolation at the end point of a non-cyclic grid
    a = AC.steering(pos, np.deg2rad(-80.0))
    got = _same(pos, (-np.pi / 3, 0.0, 91), np.outer(a, a.conj()))
    assert got["grid_idx"] == 0 and got["az_rad"] == float(np.float32(-np.pi / 3))


# ---------------------------------------------------------------- 2. interpolation bias
def _bias_deg(pos, scan, az_deg):
    worst = 0.0
    for d in az_deg:
        a = AC.steering(pos, np.deg2rad(d))
        worst = max(worst, AC.ang_err_deg(AC.estimate(pos, *scan, np.outer(a, a.conj()))["az_rad"], d))
    return worst


def test_interpolation_bias():
    az = np.arange(-75.0, 75.0001, 0.137)
    worst = max(_bias_deg(AC.ula(n), AC.SCAN_ULA, az) for n in (2, 4, 8))
    print(f"aoa interpolation bias, 181 points over +-90 deg: {worst:.4f} deg; "
          f"91 points {_bias_deg(AC.ula(4), (AC.SCAN_ULA[0], AC.SCAN_ULA[1], 91), az):.4f}, "
          f"361 points {_bias_deg(AC.ula(4), (AC.SCAN_ULA[0], AC.SCAN_ULA[1], 361), az):.4f}")
    assert worst <= AC.BIAS_CAP_DEG["ula"]
    assert worst <= AC.BIAS_DEG["ula"] * 1.01  # the recorded figure the GPU test's bound uses
    uca = _bias_deg(AC.uca(8), AC.SCAN_UCA, np.arange(-180.0, 180.0, 0.731))
    print(f"aoa interpolation bias, cyclic 360 points on the circle: {uca:.5f} deg")
    assert uca <= AC.BIAS_CAP_DEG["uca"]
    assert uca <= AC.BIAS_DEG["uca"] * 1.01 + 5e-5


# ---------------------------------------------------------------- 3. / 4. the noisy inputs are decidable
def _noisy(name, **wrong):
    g = AC.geometry(name)
    errs = []
    for w in AC.windows(name, snr_db=AC.NOISY_SNR_DB):
        R = AC.model_cov(g, w["win"], w["off"], swap=wrong.get("swap"))
        est = AC.estimate(g["pos"], *g["scan"], R, conj=wrong.get("conj", False))
        errs.append(AC.ang_err_deg(est["az_rad"], w["az_deg"]))
    return max(errs)


@pytest.mark.parametrize("name", AC.MODEL_CASES)
def test_noisy_inputs_are_decidable(name):
    err = _noisy(name)
    print(f"aoa noisy {name}: model az - truth {err:.3f} deg, recorded {AC.NOISY_ERR_DEG[name]:.3f}")
    assert err <= 2.0 * AC.NOISY_ERR_DEG[name]


@pytest.mark.parametrize("name", AC.MODEL_CASES)
def test_wrong_models_miss_the_bound(name):
    bound = 2.0 * AC.NOISY_ERR_DEG[name]
    assert _noisy(name, conj=True) > bound
    assert _noisy(name, swap=(0, 1)) > bound


def test_noiseless_model_is_rank_one():
    for name in AC.MODEL_CASES:
        g = AC.geometry(name)
        for w in AC.windows(name):
            R = AC.model_cov(g, w["win"], w["off"])
            a = AC.steering(g["pos"], np.deg2rad(w["az_deg"]))
            d = np.linalg.norm(R / np.trace(R).real - np.outer(a, a.conj()) / g["n_rx"])
            assert d <= 1e-6, (name, d)  # complex64 windows


# ---------------------------------------------------------------- 5. refusals
def test_einval():
    L = dnrp.lib()
    cfg = dnrp._aoa_cfg(AC.ula(4), *AC.SCAN_ULA)
    assert L.dnrp_ctx_set_rx_aoa(None, C.byref(cfg)) == EINVAL
    assert L.dnrp_ctx_set_rx_aoa(None, None) == EINVAL
    on = C.c_uint32()
    assert L.dnrp_ctx_get_rx_aoa(None, C.byref(on), None) == EINVAL
    out = dnrp.AoaReport()
    assert L.dnrp_rx_aoa(None, 1, C.byref(out), None) == EINVAL
    R = np.zeros((8, 8), np.complex64)
    Rp = C.c_void_p(R.ctypes.data)
    assert L.dnrp_aoa_estimate(C.byref(cfg), 4, Rp, C.byref(out), None) == 0
    assert L.dnrp_aoa_estimate(None, 4, Rp, C.byref(out), None) == EINVAL
    assert L.dnrp_aoa_estimate(C.byref(cfg), 4, None, C.byref(out), None) == EINVAL
    assert L.dnrp_aoa_estimate(C.byref(cfg), 4, Rp, None, None) == EINVAL
    for n in (0, 1, 9):
        assert L.dnrp_aoa_estimate(C.byref(cfg), n, Rp, C.byref(out), None) == EINVAL
    pi = float(np.pi)
    bad = [dict(n_grid=7), dict(n_grid=513), dict(az_min=1.0, az_max=1.0), dict(az_min=1.0, az_max=0.5),
           dict(az_min=-pi, az_max=pi + 1e-3), dict(az_min=float("nan")), dict(az_max=float("inf")), dict(reserved=1),
           dict(pos=float("nan")), dict(pos7=float("inf"))]
    for b in bad:
        c = dnrp._aoa_cfg(AC.ula(4), *AC.SCAN_ULA)
        for k, v in b.items():
            if k == "pos":
                c.pos[1][0] = v
            elif k == "pos7":
                c.pos[7][1] = v
            else:
                setattr(c, k, v)
        assert L.dnrp_aoa_estimate(C.byref(c), 4, Rp, C.byref(out), None) == EINVAL, b
    # the widest grids are accepted
    for n_grid in (8, 512):
        spec = dnrp.aoa_estimate(AC.uca(8), -pi, pi, n_grid, np.eye(8))["spectrum"]
        assert spec.shape == (n_grid,) and np.allclose(spec, 1.0 / 8.0, atol=1e-6)
