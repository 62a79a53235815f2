"""Virtual space and channel scanner on a machine without a GPU: dnrp_vspace_mix and dnrp_chscan_batch
refuse a NULL context before any device call, and the ctypes mirrors of their structures have the sizes
include/dnrp.h lays out."""
import ctypes as C

import pytest

dnrp = pytest.importorskip("dnrp")


def test_null_context_is_einval():
    L = dnrp.lib()
    cfg = dnrp.ChannelCfg(dnrp.CH_AWGN, 0, 0.0, 0.0, 1, 1.0, 10.0, 1.0, 1)
    assert L.dnrp_vspace_mix(None, C.byref(cfg), None, 0, None, 1, None, 0, 0, 1, None, 16, 16, 0, 16, None) == -1
    assert L.dnrp_vspace_mix(None, None, None, 0, None, 0, None, 0, 0, 0, None, 0, 0, 0, 0, None) == -1
    req = dnrp.ChscanReq(99, 10, 2, 1)
    avg, part, off = C.c_float(), (C.c_float * 2)(), C.c_uint32(0)
    assert L.dnrp_chscan_batch(None, None, 100, 100, 1, 1, C.byref(req), part, C.byref(off), C.byref(avg), None) == -1
    assert L.dnrp_chscan_batch(None, None, 0, 0, 0, 0, None, None, None, None, None) == -1


def test_structure_sizes():
    assert C.sizeof(dnrp.VspaceEmission) == 32
    assert C.sizeof(dnrp.AdcCfg) == 8
    assert C.sizeof(dnrp.ChscanReq) == 24
    assert dnrp.ChscanReq(5, 2).N_ant == 2 ** 32 - 1  # unset: every antenna of the ring (chscanner.cpp:43)
