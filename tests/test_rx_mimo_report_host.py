"""The MIMO report options on the host (dnrp_ctx_set_rx_mimo_report, dnrp_rx_mimo_detail): the numpy model of
tests/mimo_report_cases.py against hand-computed examples and known channels, the argument checks that need no
device, the structure's size, and the conditions on the seeds the GPU test relies on."""
import ctypes as C

import numpy as np
import pytest

import mimo_report_cases as MR

EINVAL = -1
R2 = float(np.float32(1.0) / np.sqrt(np.float32(2.0)))  # the table's scaling factor, a float


def test_model_reproduces_the_oracle_loopback_rank_one_pick():
    """test_oracle_loopback.test_mimo_report_codebook_search: H = g conj(w)^T, w entry 17 of the 4-antenna
    single-stream codebook; the oracle reports 17 under the reference's default metric"""
    w = np.array([1, 1j, 1j, -1]) / 2
    g = np.array([1.0, 0.9, 1.1, 0.95])
    H = MR.stage_of(np.outer(g, np.conj(w)))
    idx, scores, margin = MR.search(H, "tx", 0, 0)
    assert idx == 17 and margin > 0
    assert np.all(np.isnan(scores[:12])) and np.all(np.isfinite(scores[12:]))
    # entry 17 scores min_rx |g| * 4 cells * |w^H w| / scaling: 0.9 * 4 * 2 * 0.5
    assert scores[17] == pytest.approx(0.9 * 4 * 2 * 0.5, rel=1e-12)


# effective 2 x 2 stages (the sum over the 4 cells), the codebook (1, 2) = (1,0) (0,1) (1,1) (1,-1) (1,j) (1,-j) with
# scaling 1, 1, then 1/sqrt2: per entry the two receive-side magnitudes are
#   A = [[2,0],[2,0]]: (2,2) (0,0) (2,2) (2,2) (2,2) (2,2)
#   B = [[3,1],[1,1]]: (3,1) (1,1) (4,2) (2,0) (sqrt10,sqrt2) (sqrt10,sqrt2)
S10 = np.sqrt(10.0)
HAND = {
    "A": (np.array([[2, 0], [2, 0]], float), {
        0: [2, 0, 2 * R2, 2 * R2, 2 * R2, 2 * R2],
        1: [4, 0, 4 * R2, 4 * R2, 4 * R2, 4 * R2],
        2: [0, 0, 0, 0, 0, 0]},
        # (metric, all_w): index -- the non-zero entries tie, the first (2) wins; metric 2 ties everywhere
        {(0, 0): 2, (0, 1): 0, (1, 0): 2, (1, 1): 0, (2, 0): 2, (2, 1): 0}),
    "B": (np.array([[3, 1], [1, 1]], float), {
        0: [1, 1, 2 * R2, 0, np.sqrt(2.0) * R2, np.sqrt(2.0) * R2],
        1: [4, 2, 6 * R2, 2 * R2, (S10 + np.sqrt(2.0)) * R2, (S10 + np.sqrt(2.0)) * R2],
        2: [2, 0, 2 * R2, 2 * R2, (S10 - np.sqrt(2.0)) * R2, (S10 - np.sqrt(2.0)) * R2]},
        # metric 2: entries 4 and 5 tie at the smallest spread of the non-zero entries, 4 wins; entry 1 has none
        {(0, 0): 2, (0, 1): 2, (1, 0): 2, (1, 1): 2, (2, 0): 4, (2, 1): 1}),
}


@pytest.mark.parametrize("name", sorted(HAND))
@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("all_w", [0, 1])
def test_hand_computed_2x2(name, metric, all_w):
    Heff, scores, picks = HAND[name]
    H = MR.stage_of(Heff / 4.0)
    idx, sc, _ = MR.search(H, "tx", metric, all_w)
    A = 0 if all_w else 2
    assert np.all(np.isnan(sc[:A])) and np.all(np.isnan(sc[6:]))
    assert np.allclose(sc[A:6], scores[metric][A:], rtol=0, atol=1e-12)
    assert idx == picks[(metric, all_w)]
    assert MR.first_best(sc, metric) == idx
    # the reciprocal side searches the transposed stage
    idr, scr, _ = MR.search(np.transpose(H, (1, 0, 2)), "rx", metric, all_w)
    assert idr == idx and np.array_equal(scr, sc, equal_nan=True)


def test_trivial_and_missing_codebooks():
    H = MR.stage_of(MR.gauss(0, 8, 1))
    assert MR.search(H, "tx", 0, 0)[0] == 0 and np.all(np.isnan(MR.search(H, "tx", 0, 0)[1]))
    assert MR.search(H, "rx", 0, 0)[0] == MR.NONE and np.all(np.isnan(MR.search(H, "rx", 1, 1)[1]))
    assert np.all(np.isnan(MR.rates(MR.stage_of(MR.gauss(0, 8, 8)), 0.01)))  # no codebook at N_TS = 8
    r = MR.rates(H, 0.01)
    assert np.isfinite(r[0, 0]) and np.all(np.isnan(r[0, 1:])) and np.all(np.isnan(r[1:]))


@pytest.mark.parametrize("n_tx,n_rx,cb", [(4, 4, 17), (2, 2, 3), (4, 4, 12), (2, 4, 5)])
def test_rank_one_channel(n_tx, n_rx, cb):
    g = MR.gauss(3, n_rx, 1)[:, 0]
    H = MR.stage_of(MR.rank_one(g / np.abs(g), n_tx, cb))
    for metric in (0, 1):
        assert MR.search(H, "tx", metric, 0)[0] == cb
    pmi, rate, RI, PMI, sinr, _ = MR.report(MR.rates(H, 0.01))
    assert RI == 1 and PMI == cb and pmi[0] == cb
    # one layer through the matched entry: |g|^2 = n_rx over the noise variance (the scaling factors are floats)
    assert rate[0] == pytest.approx(np.log2(1.0 + n_rx / 0.01), rel=1e-6)
    assert sinr == pytest.approx(10.0 * np.log10(n_rx / 0.01), abs=1e-5)


@pytest.mark.parametrize("n", [2, 4])
def test_unitary_channel_takes_every_layer(n):
    pmi, rate, RI, PMI, _, _ = MR.report(MR.rates(MR.stage_of(MR.unitary(n)), 0.01))
    assert RI == n and PMI == pmi[{2: 1, 4: 2}[n]]
    assert rate[{2: 1, 4: 2}[n]] == pytest.approx(n * np.log2(1.0 + 1.0 / n / 0.01), rel=1e-6)


def test_noise_floor():
    H = MR.stage_of(np.full((2, 2), 2.0))
    assert MR.nv_used(0.0, H, 2, 2) == 4.0 * 2.0 ** -14
    assert MR.nv_used(0.5, H, 2, 2) == 0.5
    assert MR.nv_used(0.0, np.zeros((2, 2, 4)), 2, 2) == float(np.finfo(np.float32).tiny)


def test_entry_points_refuse_a_null_context():
    import dnrp
    L = dnrp.lib()
    for n in ("dnrp_ctx_set_rx_mimo_report", "dnrp_ctx_get_rx_mimo_report", "dnrp_rx_mimo_detail"):
        assert n in dnrp.EXPORTS
    row = dnrp.MimoDetail()
    u = C.c_uint32()
    assert L.dnrp_ctx_set_rx_mimo_report(None, 0, 0, 0) == EINVAL
    assert L.dnrp_ctx_get_rx_mimo_report(None, C.byref(u), C.byref(u), C.byref(u)) == EINVAL
    assert L.dnrp_rx_mimo_detail(None, 1, C.byref(row), None) == EINVAL


def test_structure_size():
    import dnrp
    cb = dnrp.MIMO_MAX_CB
    words = 2 + 8 * 8 * 4 * 2 + 2 + 2 + 2 * cb + 2 + 3 + 3 + 3 * cb + 1
    assert C.sizeof(dnrp.MimoDetail) == 4 * words == dnrp.MIMO_DETAIL_DTYPE.itemsize
    assert cb == 28 == max(int(dnrp.query_table("W_codebooks", r, n)[0]) for r, n in ((1, 1), (1, 2), (1, 4), (2, 2), (2, 4), (4, 4)))
    assert dnrp.MimoDetail.H.offset == 8 and dnrp.MimoDetail.sinr_eff_dB.offset == 4 * (words - 1)
    assert dnrp.MIMO_DETAIL_DTYPE.fields["rate_cb"][1] == dnrp.MimoDetail.rate_cb.offset


# ---------------------------------------------------------------- the seeds the GPU test uses
def _decisions(name):
    """per packet of the geometry's batch, on the mixing itself as the stage at nv = 0.01: the picks
    {(side, metric, all_w): index} and the relative top-two margins of the index and of the rate decisions"""
    g = MR.geometry(name)
    out = []
    for s in range(MR.N_PACKETS):
        H = MR.stage_of(MR.gauss(s, g["n_rx"], g["n_tx"]))
        picks, idx_margins = {}, []
        for side in ("tx", "rx"):
            for metric in (0, 1, 2):
                for all_w in (0, 1):
                    idx, sc, m = MR.search(H, side, metric, all_w)
                    picks[(side, metric, all_w)] = idx
                    if np.isfinite(sc).any():
                        idx_margins.append(m if np.isinf(m) else m / np.nanmax(np.abs(sc)))
        rc = MR.rates(H, 0.01)
        rate_margins = [m / np.nanmax(rc) for m in MR.report(rc)[5] if np.isfinite(m)]
        out.append((picks, idx_margins, rate_margins))
    return g, out


@pytest.mark.parametrize("name", MR.BATCH_GEOMETRIES)
def test_seed_conditions(name):
    g, dec = _decisions(name)
    im = [m for _, ims, _ in dec for m in ims]
    rm = [m for _, _, rms in dec for m in rms]
    assert im and np.mean(np.array(im) < MR.SCORE_CAP) < 0.10, (name, sorted(im)[:4])
    assert not rm or np.mean(np.array(rm) < MR.RATE_CAP) < 0.10, (name, sorted(rm)[:4])
    # an ignored option cannot pass: within the batch every metric pair and the two search starts pick apart on
    # some side. With a single antenna on the receive side of a search, the minimum and the sum coincide
    sides = [sd for sd, n_txv, n_rxv in (("tx", g["n_ts"], g["n_rx"]), ("rx", g["n_rx"], g["n_ts"])) if n_txv in (2, 4)]
    assert sides
    col = lambda metric, all_w: [p[(sd, metric, all_w)] for p, _, _ in dec for sd in sides]
    pairs = [(0, 1), (0, 2), (1, 2)] if min(g["n_ts"], g["n_rx"]) > 1 or len(sides) > 1 else [(0, 2), (1, 2)]
    for a, b in pairs:
        assert col(a, 0) != col(b, 0), (name, a, b)
    for metric in (0, 1, 2):
        assert col(metric, 0) != col(metric, 1), (name, metric)
