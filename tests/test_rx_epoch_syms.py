"""The epoch receiver's symbol ownership (geometry.cpp rx_epoch_syms, read through dnrp_query_table
"rx_epoch_syms"): host logic, no GPU.

rx_epoch_kernel runs the front end of an epoch's symbols in the workgroup that equalises the epoch, so
every symbol the PDC phase still has to transform -- bearing PDC cells, after the PCC phase's last symbol,
not a DRS symbol (those go through the DRS pass ahead of it) -- must belong to exactly one epoch, and to
one whose segments read it. Checked against the plan ("rx_plan_epochs", "rx_plan_segs") and the cell maps
("symbol_cells", "pdc_cells") for the geometries of test_rx_plan_twin.py and for the packets of
test_gpu_eq_twin.py, which must qualify: the GPU test runs the epoch kernel on them.
"""
import numpy as np
import pytest

import dnrp

B = 1
N_DFS = (19, 21, 29, 34)
MODES = [(1, 1), (1, 2), (1, 3), (0, 2)]  # (mode_lr, stride)
OP_PDC = 4


def _phase(nt_s, nt, n_df, lr, stride):
    """ok, per-epoch symbol lists, DRS list of the query; the plan's epochs as lists of segment rows
    (kind, j0, j1); per symbol its PCC / PDC / DRS cell counts; per PDC cell its symbol."""
    out = dnrp.query_table("rx_epoch_syms", B, nt_s, nt, n_df, lr, stride).astype(np.int64)
    plan = (B, nt_s, nt, n_df, lr, stride, 0)
    eps = dnrp.query_table("rx_plan_epochs", *plan).astype(np.int64).reshape(-1, 3)
    segs = dnrp.query_table("rx_plan_segs", *plan).astype(np.int64).reshape(-1, 12)
    counts = dnrp.query_table("symbol_cells", B, nt_s, nt, n_df).astype(np.int64).reshape(-1, 3)
    cell_sym = dnrp.query_table("pdc_cells", B, nt_s, nt, n_df).astype(np.int64).reshape(-1, 2)[:, 0]
    ok, at, lists = bool(out[0]), 1, []
    for _ in eps:
        n = int(out[at])
        lists.append([int(l) for l in out[at + 1:at + 1 + n]])
        at += 1 + n
    drs = [int(l) for l in out[at:]]
    epochs = [[(int(s[1]), int(s[3]), int(s[4])) for s in segs[s0:s1]] for s0, s1, _ in eps]
    return ok, lists, drs, epochs, counts, cell_sym


def _check(nt_s, nt, n_df, lr, stride, must_be_ok=False):
    ok, lists, drs, epochs, counts, cell_sym = _phase(nt_s, nt, n_df, lr, stride)
    assert len(counts) == n_df + 1
    pm = max(l for l in range(n_df + 1) if counts[l, 0] > 0)
    is_drs = counts[:, 2] > 0
    mine = [l for l in range(pm + 1, n_df + 1) if counts[l, 1] > 0 and not is_drs[l]]

    # what the plan itself says: the symbols each epoch's segments read, and whether all are PDC segments
    reads = [{l for kind, j0, j1 in ep if kind == OP_PDC for l in set(cell_sym[j0:j1].tolist()) if l in mine}
             for ep in epochs]
    all_pdc = all(kind == OP_PDC for ep in epochs for kind, _, _ in ep)
    claims = np.zeros(n_df + 1, int)
    for r in reads:
        for l in r:
            claims[l] += 1

    assert len(lists) == len(epochs)
    for e, ls in enumerate(lists):
        assert ls == sorted(set(ls))
        for l in ls:  # every listed symbol overlaps a segment of its epoch
            assert any(np.any(cell_sym[j0:j1] == l) for _, j0, j1 in epochs[e]), (e, l)
            assert l in mine, (e, l)
    assert drs == [l for l in range(pm + 1, n_df + 1) if is_drs[l]]
    if ok:
        listed = np.zeros(n_df + 1, int)
        for ls in lists:
            for l in ls:
                listed[l] += 1
        assert [l for l in range(n_df + 1) if listed[l]] == mine
        assert np.all(listed[mine] == 1)
    else:
        assert not must_be_ok, (nt_s, nt, n_df, lr, stride)
        assert not all_pdc or np.any(claims > 1), "rejected without a double claim or a non-PDC segment"


@pytest.mark.parametrize("lr,stride", MODES)
@pytest.mark.parametrize("nt", [1, 2, 4])
@pytest.mark.parametrize("n_df", N_DFS)
def test_epoch_symbols(nt, n_df, lr, stride):
    _check(nt, nt, n_df, lr, stride)


@pytest.mark.parametrize("lr,stride", [(1, 2), (1, 3), (0, 2)])
@pytest.mark.parametrize("tm", [0, 1, 5])
def test_epoch_symbols_of_the_gpu_twin_cases(tm, lr, stride):
    """psdef (u 8, b 1, type 0, length 6) of tests/test_gpu_eq_twin.py: the epoch kernel runs there."""
    sz = dnrp.compute_packet_sizes(dnrp.psdef(8, 1, 0, 6, tm, 8))
    _check(sz["N_TS"], sz["N_eff_TX"], sz["N_DF_symb"], lr, stride, must_be_ok=True)


def test_query_arguments():
    with pytest.raises(dnrp.DnrpError):
        dnrp.query_table("rx_epoch_syms", B, 4, 4, 34, 1, 0)  # stride 0
    with pytest.raises(dnrp.DnrpError):
        dnrp.query_table("rx_epoch_syms", B, 4, 4, 34, 1)
