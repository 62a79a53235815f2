"""The one-wavefront FFT's exchange slots and the front end's mixer stores, on the host, from the kernels' own
index header.

csrc/kernels/wfft_index.hpp holds the index arithmetic that wave_fft1024 / wave_fft1024_rt (device_common.hpp)
and rx_span / rx_resample_ct (rx_front.hpp) call: the four access patterns' lane bases and offsets, the
closed-form slot wfft_pad(i0) + wfft_off(c), a symbol's polyphase blocks and the slot of a block's first
mixer store. tests/wfft_index_dump.cpp includes that header, is compiled here with the system's C++ compiler
and prints what the header computes; this file checks it.

  * Exchange slots: for all 64 lanes and every offset of the four patterns (k, r < 16; b, r < 4) the closed
    form equals i + (i >> 4) of the element index, every slot lies inside WFFT_XB, and every pattern
    touches each of the 1024 elements once.
  * Mixer stores: for every data symbol of a mu = 8, beta = 16 and a mu = 1, beta = 16 packet at 10/9 and
    every block alignment m_star < 9, only the first and the last block of the symbol hold outputs outside
    [m0, m0 + 1024); with the pad every store of every block lands in [0, 1024 + 2 pad) of the region, a
    round's stores stay below the next round's windows, the blocks fit the kernel's rounds, and the
    symbol's 1024 outputs are each stored once.
"""
import functools
import os
import shutil
import subprocess

import pytest

import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = os.path.join(HERE, "..", "dect-nr-plus-sdr_amd", "csrc", "kernels")
LR, MR = 9, 10  # the front end's 9/10 resampler (taps_rx_9_10)


@functools.lru_cache(maxsize=None)
def _tool():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a C++ compiler (the one that builds oracle/) is needed"
    import tempfile
    out = os.path.join(tempfile.mkdtemp(prefix="wfft_index_"), "wfft_index_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", KERNELS, os.path.join(HERE, "wfft_index_dump.cpp"), "-o", out], check=True)
    return out


def _run(*args):
    return subprocess.run([_tool(), *map(str, args)], check=True, capture_output=True, text=True).stdout.split("\n")


def test_exchange_slot_identities():
    lines = _run("slots")
    head = lines[0].split()
    xb, pad = int(head[1]), int(head[3])
    assert xb == 1088 and pad == LR - 1
    seen = {p: [] for p in ("w1", "r2", "w2", "r3")}
    count = {p: 0 for p in seen}
    for ln in lines[1:]:
        if not ln:
            continue
        p, lane, n, i, slot = ln.split()
        lane, n, i, slot = int(lane), int(n), int(i), int(slot)
        assert slot == i + (i >> 4), ln  # the closed form is the padded index of the element
        assert 0 <= slot < xb, ln
        seen[p].append(i)
        count[p] += 1
    for p in seen:  # 64 lanes x 16 accesses: every element once
        assert count[p] == 1024 and sorted(seen[p]) == list(range(1024)), p
    assert len({i + (i >> 4) for i in range(1024)}) == 1024


@pytest.mark.parametrize("u", [8, 1])
def test_mixer_store_blocks(u):
    ocf, ops = O.cfg(u, 16, 1, 10, 9), O.psdef(u, 16, 1, 1, 0, 1)
    sz, dm = O.packet_sizes(ops), O.dims(ocf, ops)
    assert dm["N_b_DFT_os"] == 1024
    n_sym = sz["N_DF_symb"]
    assert n_sym >= 4
    lines = _run("blocks", dm["STF_CP_os"], dm["CP_os"], n_sym)
    rounds = int(lines[0].split()[1])
    pad = LR - 1
    syms, cur = [], None
    for ln in lines[1:]:
        f = ln.split()
        if not f:
            continue
        if f[0] == "sym":
            cur = dict(m_star=int(f[1]), l=int(f[2]), m0=int(f[3]), qb0=int(f[4]), qb1=int(f[5]), blk=[])
            syms.append(cur)
        else:
            cur["blk"].append((int(f[1]), int(f[2])))
    assert len(syms) == LR * n_sym
    n_stf, cp = dm["STF_CP_os"] + 1024, dm["CP_os"]
    for s in syms:
        assert s["m0"] == n_stf + (s["l"] - 1) * (cp + 1024) + cp  # the symbol's first output behind its CP
        qb0, qb1 = s["qb0"], s["qb1"]
        assert [q for q, _ in s["blk"]] == list(range(qb0, qb1))
        assert qb1 - qb0 <= 64 * rounds
        stored = []
        for q, slot0 in s["blk"]:
            idx = [s["m_star"] + LR * q + k - s["m0"] for k in range(LR)]  # the block's outputs relative to m0
            assert slot0 == idx[0] + pad, (s, q)
            if any(not 0 <= i < 1024 for i in idx):
                assert q in (qb0, qb1 - 1), (u, s["m_star"], s["l"], q)
            assert 0 <= slot0 and slot0 + LR - 1 < 1024 + 2 * pad
            if q - qb0 < 64:  # round 0: below the windows of round 1 (block qb0 + 64 reads from R[MR * 64])
                assert slot0 + LR - 1 < MR * 64
            stored += idx
        assert sorted(i for i in stored if 0 <= i < 1024) == list(range(1024))
