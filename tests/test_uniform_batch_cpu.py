"""Uniform xdp batches on the host side (no GPU): XDPBatch.from_numpy drops pkt_off / pkt_len only
when the host array it was handed proves them redundant (offsets off[0] + i * s with 0 < s < 2^32,
lengths all equal, n > 1), the mimic_xdp_batch struct then carries NULL arrays and the two scalars
(include/mimic_amd.h), and both owned kernels still build within test_own_budget_cpu.py's limits."""
import numpy as np
import pytest

import mimic_amd as M
from mimic_amd import jit
from mimic_amd import workloads as W


def _mk(n, stride=64, length=64, base=0, seed=1):
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, base + max(n, 1) * stride + 64, dtype=np.uint8)
    off = (base + np.arange(n, dtype=np.uint64) * np.uint64(stride)).astype(np.uint64)
    lens = np.full(n, length, dtype=np.uint32)
    return buf, off, lens


def _struct(b):
    b._c()
    return b._cstruct_obj


def test_uniform_offsets_and_lengths_drop_both_arrays():
    buf, off, lens = _mk(100, stride=96, length=60)
    b = M.XDPBatch.from_numpy(buf, off, lens, device="cpu")
    assert b.pkt_off is None and b.pkt_len is None
    assert (b.n, b.pkt_stride, b.pkt_len_all, b.pkt_base) == (100, 96, 60, 0)
    c = _struct(b)
    assert c.n == 100 and not c.pkt_off and not c.pkt_len
    assert (c.pkt_stride, c.pkt_len_all) == (96, 60)
    assert c.pkt_data == b.pkt_data.data_ptr()


def test_first_offset_is_folded_into_the_data_pointer():
    buf, off, lens = _mk(10, stride=128, length=64, base=200)
    b = M.XDPBatch.from_numpy(buf, off, lens, device="cpu")
    assert b.pkt_off is None and b.pkt_base == 200
    c = _struct(b)
    assert c.pkt_data == b.pkt_data.data_ptr() + 200 and c.pkt_stride == 128
    assert [b.offset(i) for i in (0, 1, 9)] == [200, 328, 200 + 9 * 128]
    assert np.array_equal(b.offsets(), off.astype(np.int64))


def test_one_length_different_drops_only_pkt_off():
    buf, off, lens = _mk(50)
    lens[17] = 63
    b = M.XDPBatch.from_numpy(buf, off, lens, device="cpu")
    assert b.pkt_off is None and b.pkt_len is not None
    c = _struct(b)
    assert not c.pkt_off and c.pkt_len == b.pkt_len.data_ptr()
    assert (c.pkt_stride, c.pkt_len_all) == (64, 0)
    assert b.length(17) == 63 and b.length(16) == 64


@pytest.mark.parametrize("how", ["one_byte", "descending", "zero_stride", "stride_2_32"])
def test_irregular_offsets_keep_pkt_off(how):
    buf, off, lens = _mk(20)
    if how == "one_byte":
        off[11] += 1
    elif how == "descending":
        off[0], off[1] = off[1], off[0]
    elif how == "zero_stride":
        off[:] = 64
    else:
        off = np.arange(20, dtype=np.uint64) * np.uint64(1 << 32)
    b = M.XDPBatch.from_numpy(buf, off, lens, device="cpu")
    assert b.pkt_off is not None and b.pkt_len is None
    assert np.array_equal(b.pkt_off.numpy().view(np.uint64), off)
    c = _struct(b)
    assert c.pkt_off == b.pkt_off.data_ptr() and c.pkt_stride == 0 and not c.pkt_len and c.pkt_len_all == 64
    assert c.pkt_data == b.pkt_data.data_ptr()


def test_last_offset_wrong_keeps_pkt_off():
    buf, off, lens = _mk(20)
    off[19] -= 1
    assert M.XDPBatch.from_numpy(buf, off, lens, device="cpu").pkt_off is not None


@pytest.mark.parametrize("n", [0, 1])
def test_tiny_batches_keep_their_arrays(n):
    buf, off, lens = _mk(n)
    b = M.XDPBatch.from_numpy(buf, off, lens, device="cpu")
    assert b.pkt_off is not None and b.pkt_len is not None and b.n == n
    c = _struct(b)
    assert c.n == n and c.pkt_stride == 0 and c.pkt_len_all == 0


def test_constructor_keeps_what_it_is_given():
    import torch

    buf, off, lens = _mk(30)
    t_off, t_len = torch.from_numpy(off.view(np.int64)), torch.from_numpy(lens.view(np.int32))
    b = M.XDPBatch(torch.from_numpy(buf), t_off, t_len)
    assert b.pkt_off is t_off and b.pkt_len is t_len and b.n == 30
    c = _struct(b)
    assert c.pkt_off == t_off.data_ptr() and c.pkt_len == t_len.data_ptr() and c.pkt_stride == 0 and c.pkt_len_all == 0
    # the compact forms, each alone and both, as given
    b = M.XDPBatch(torch.from_numpy(buf), None, t_len, pkt_stride=64)
    c = _struct(b)
    assert b.n == 30 and not c.pkt_off and c.pkt_len == t_len.data_ptr() and c.pkt_stride == 64
    b = M.XDPBatch(torch.from_numpy(buf), t_off, None, pkt_len_all=64)
    c = _struct(b)
    assert b.n == 30 and c.pkt_off == t_off.data_ptr() and not c.pkt_len and c.pkt_len_all == 64
    b = M.XDPBatch(torch.from_numpy(buf), None, None, pkt_stride=64, pkt_len_all=64, n=30)
    c = _struct(b)
    assert c.n == 30 and not c.pkt_off and not c.pkt_len
    with pytest.raises(ValueError):
        M.XDPBatch(torch.from_numpy(buf), None, None, pkt_stride=64, pkt_len_all=64)   # no n
    with pytest.raises(ValueError):
        M.XDPBatch(torch.from_numpy(buf), t_off, None, pkt_len_all=64, n=31)


def test_knob_keeps_every_array(monkeypatch):
    monkeypatch.setenv("MIMIC_BATCH_COMPACT", "0")
    buf, off, lens = _mk(100)
    b = M.XDPBatch.from_numpy(buf, off, lens, device="cpu")
    assert b.pkt_off is not None and b.pkt_len is not None
    c = _struct(b)
    assert c.pkt_off and c.pkt_len and c.pkt_stride == 0 and c.pkt_len_all == 0


def test_from_packets_detects_too():
    b = M.XDPBatch.from_packets([bytes([i]) * 60 for i in range(8)], device="cpu")
    assert b.pkt_off is None and b.pkt_len is None and (b.pkt_stride, b.pkt_len_all) == (64, 60)
    b = M.XDPBatch.from_packets([bytes([i]) * (60 + 70 * (i == 3)) for i in range(8)], device="cpu")
    assert b.pkt_off is not None and b.pkt_len is not None


@pytest.mark.parametrize("headroom,tailroom", [(0, 0), (8, 24)])
def test_packet_bytes_agrees_between_the_forms(monkeypatch, headroom, tailroom):
    buf, off, lens = _mk(40, stride=128, length=64, base=64)
    a = M.XDPBatch.from_numpy(buf, off, lens, device="cpu", headroom=headroom, tailroom=tailroom)
    monkeypatch.setenv("MIMIC_BATCH_COMPACT", "0")
    k = M.XDPBatch.from_numpy(buf, off, lens, device="cpu", headroom=headroom, tailroom=tailroom)
    assert a.pkt_off is None and k.pkt_off is not None
    for i in (0, 1, 17, 39):
        want = bytes(buf[int(off[i]):int(off[i]) + headroom + 64 + tailroom])
        assert a.packet_bytes(i) == k.packet_bytes(i) == want


def test_ctypes_struct_matches_the_header():
    """The two scalars are appended: every earlier field keeps its offset."""
    from mimic_amd import _lib

    f = {n: getattr(_lib.XDPBatch, n).offset for n, _ in _lib.XDPBatch._fields_}
    assert f["cpu"] == 112 and f["step_budget"] == 120 and f["pkt_stride"] == 128 and f["pkt_len_all"] == 132
    import ctypes

    assert ctypes.sizeof(_lib.XDPBatch) == 136
    # the ABI version did not move with the struct: the library tells its own size
    assert _lib.load().mimic_xdp_batch_size() == 136


@pytest.mark.parametrize("prog", ["prog_classifier", "prog_parse5"])
def test_owned_kernels_build_within_the_budget(prog):
    p = getattr(W, prog)()
    src = jit.kernel_source([p.raw], 0, (), jit.spread_spec([(p.raw, p.relocs)], p.maps, 262144, own=True))
    assert "pkt_off_pf(" in src and "pkt_off_take(" in src   # the owned form reads descriptors through the accessors
    r = jit.kernel_resources(jit.code_object(src))
    assert r["vgpr_total"] <= 128 and r["waves_per_simd"] == 4
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0
    assert r["sgpr_spill"] < 68
