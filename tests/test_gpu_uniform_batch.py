"""Uniform xdp batches on MI355X: mimic_xdp_batch with pkt_off and / or pkt_len NULL (packet memory
i at pkt_data + i * pkt_stride, every length pkt_len_all) on every engine -- the owned spread
kernel, the table spread, the one-lane JIT and the batch interpreter -- against the oracle (R0,
status, steps, err_pc, packet memory, every map byte) and, bit for bit, against the same batch
given with its arrays.  The shapes sit where the index arithmetic can go wrong: one packet, fewer
packets than lanes, a partial last row, exactly lanes * P, both schedules, strides with gaps and
off the 64-byte grid, scalar rooms; mimic_run_xdp_many with the forms mixed in one launch."""
import ctypes as C

import numpy as np
import pytest

import mimic_amd as M
from harness import Scenario, build_engine, build_oracle, kernel_of, ncpus, run_oracle, spread_kernel_of
from mimic_amd import _lib
from mimic_amd import asm as A
from mimic_amd import workloads as W

pytestmark = pytest.mark.gpu

VS = (8, 64, 256)


def _sc(p, V):
    return Scenario(vcpus=V, maps=p.maps, progs=[(p.name, p.raw, p.relocs)])


def _writer():
    """Per-CPU counter[length & 3] += 1 and a packet write: byte 7 = byte 0 + 1, when 8 bytes are there."""
    raw, rel = A.assemble([
        A.mov64_reg(6, 1), A.ldx(4, 2, 6, 0), A.ldx(4, 3, 6, 4), A.mov64_reg(4, 2), A.alu64("add", 4, 8),
        A.jmp("jgt", 4, 3, "cnt", reg=True), A.ldx(1, 5, 2, 0), A.alu64("add", 5, 1), A.stx(1, 2, 7, 5),
        "cnt", A.mov64_reg(4, 3), A.alu64("sub", 4, 2, reg=True), A.alu64("and", 4, 3), A.stx(4, 10, -4, 4),
        A.mov64_reg(2, 10), A.alu64("add", 2, -4), A.ld_map_fd(1, "c"), A.call(A.FN_MAP_LOOKUP_ELEM),
        A.jmp("jeq", 0, 0, "out"), A.ldx(8, 7, 0, 0), A.alu64("add", 7, 1), A.stx(8, 0, 0, 7),
        "out", A.mov64_imm(0, 2), A.exit_()])
    return W.Program("wr", raw, rel, [dict(name="c", type=6, key_size=4, value_size=8, max_entries=4)])


PROGS = {"classifier": W.prog_classifier, "writer": _writer}


def jit_kernels():
    out = []
    for mk in PROGS.values():
        for V in VS:
            sc = _sc(mk(), V)
            out += [spread_kernel_of(sc, own=True), spread_kernel_of(sc), kernel_of(sc)]
    return out


def _tensors(buf, off, lens, drop_off, drop_len, dev="cuda:0"):
    """The batch's device tensors in the asked form; a dropped array must be redundant."""
    import torch

    n = len(lens)
    kw = dict(n=n)
    t_off = t_len = None
    if drop_off:
        s = int(off[1]) - int(off[0]) if n > 1 else 64
        assert np.array_equal(off, off[0] + np.arange(n, dtype=np.uint64) * np.uint64(s))
        kw.update(pkt_stride=s, pkt_base=int(off[0]) if n else 0)
    else:
        t_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    if drop_len:
        assert n == 0 or (lens == lens[0]).all()
        kw.update(pkt_len_all=int(lens[0]) if n else 0)
    else:
        t_len = torch.from_numpy(lens.view(np.int32).copy()).to(dev)
    return torch.from_numpy(buf.copy()).to(dev), t_off, t_len, kw


def _batch(buf, off, lens, drop_off, drop_len, schedule, headroom=0, tailroom=0):
    data, t_off, t_len, kw = _tensors(buf, off, lens, drop_off, drop_len)
    return M.XDPBatch(data, t_off, t_len, headroom, tailroom, 1, 0, 0, schedule, **kw)


def _engine(sc, buf, off, lens, sched, drop_off, drop_len, exec_mode=None, spread=None, headroom=0, tailroom=0):
    vm, maps, pids = build_engine(sc, exec_mode=exec_mode, spread=spread)
    mode = M.SCHED_INTERLEAVED if sched == "interleaved" else M.SCHED_CHUNKED
    b = _batch(buf, off, lens, drop_off, drop_len, mode, headroom, tailroom)
    out = vm.RunXDPBatch(pids[0], b).numpy(len(lens))
    out["pkt"] = b.pkt_data.cpu().numpy()
    out["maps"] = {m["name"]: [maps[m["name"]].Values(c) for c in range(ncpus(sc, m))] for m in sc.maps}
    out["last_exec"] = vm.LastExec()
    vm.close()
    return out


def _same(a, b, what):
    for k in ("r0", "status", "steps", "err_pc"):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        x = x.astype(np.uint64) if k == "r0" else x.astype(np.int64)
        y = y.astype(np.uint64) if k == "r0" else y.astype(np.int64)
        bad = np.nonzero(x != y)[0]
        assert len(bad) == 0, f"{what}: {k} differs at {bad[:8]}: {x[bad[:8]]} vs {y[bad[:8]]}"
    assert np.array_equal(a["pkt"], b["pkt"]), f"{what}: packet memory differs"
    for name, vals in a["maps"].items():
        for c, v in enumerate(vals):
            assert v == b["maps"][name][c], f"{what}: map {name} cpu {c} differs"


def _check(prog, V, n, sched, want_exec, drop=(True, True), exec_mode=None, spread=None, headroom=0, tailroom=0,
           pk=None, **mk):
    sc = _sc(PROGS[prog](), V)
    buf, off, lens = pk if pk is not None else W.make_packets(n, seed=V + n, headroom=headroom, tailroom=tailroom, **mk)
    cpu = W.schedule_cpu(n, V, sched)
    o = run_oracle(sc, buf, off, lens, cpu, headroom=headroom, tailroom=tailroom, ingress=np.ones(n, np.int32))
    e = _engine(sc, buf, off, lens, sched, drop[0], drop[1], exec_mode, spread, headroom, tailroom)
    assert e["last_exec"] == want_exec
    _same(o, e, "oracle vs uniform batch")
    k = _engine(sc, buf, off, lens, sched, False, False, exec_mode, spread, headroom, tailroom)
    assert k["last_exec"] == want_exec
    _same(k, e, "arrays vs uniform batch")


# (V, n): one packet; fewer packets than lanes; a partial last row (P = 5); exactly lanes * P (P = 4);
# several blocks of rows (P = 12)
SHAPES = [(8, 1, "jit"), (256, 100, "jit"), (64, 64 * 4 + 13, "spread_own"), (64, 256, "spread_own"),
          (256, 3001, "spread_own")]


@pytest.mark.parametrize("prog", list(PROGS))
@pytest.mark.parametrize("sched", ["interleaved", "chunked"])
@pytest.mark.parametrize("V,n,want", SHAPES)
def test_shapes(gpu, prog, sched, V, n, want):
    _check(prog, V, n, sched, want)


@pytest.mark.parametrize("prog", list(PROGS))
@pytest.mark.parametrize("sched", ["interleaved", "chunked"])
@pytest.mark.parametrize("align", [128, 80, 200])
def test_strides_with_gaps_and_off_the_grid(gpu, prog, sched, align):
    """64-byte packets every 128 bytes (gaps), every 80 and every 200 bytes (not a multiple of 64)."""
    _check(prog, 64, 1000, sched, "spread_own", align=align)


@pytest.mark.parametrize("prog", list(PROGS))
@pytest.mark.parametrize("sched", ["interleaved", "chunked"])
def test_scalar_rooms(gpu, prog, sched):
    """Headroom 16 and tailroom 24 for every packet in 112-byte slots (H + L + T = 104): the owned
    kernel's general path, rooms zeroed in place."""
    _check(prog, 64, 777, sched, "spread_own", headroom=16, tailroom=24, align=112)


@pytest.mark.parametrize("prog", list(PROGS))
@pytest.mark.parametrize("sched", ["interleaved", "chunked"])
def test_offsets_only_with_varying_lengths(gpu, prog, sched):
    """Fixed 64-byte slots, frames of 64, 40, 20 and 7 bytes: pkt_off dropped, pkt_len kept; the
    classifier reads 34 bytes, so its bounds checks decide for the short frames."""
    _check(prog, 64, 1500, sched, "spread_own", drop=(True, False), sizes=(64, 40, 20, 7), weights=(4, 1, 1, 1))


@pytest.mark.parametrize("prog", list(PROGS))
@pytest.mark.parametrize("sched", ["interleaved", "chunked"])
def test_lengths_only_over_irregular_offsets(gpu, prog, sched):
    """Equal lengths, the slots in a shuffled order: pkt_len dropped, pkt_off kept."""
    buf, off, lens = W.make_packets(1500, seed=5, align=128)
    off = off[np.random.default_rng(9).permutation(len(off))].copy()
    _check(prog, 64, 1500, sched, "spread_own", drop=(False, True), pk=(buf, off, lens))


@pytest.mark.parametrize("prog", list(PROGS))
@pytest.mark.parametrize("sched", ["interleaved", "chunked"])
@pytest.mark.parametrize("engine", ["table", "one_lane", "interp"])
def test_other_engines(gpu, monkeypatch, prog, sched, engine):
    """The table spread (V = 64 <= packets per block), the one-lane JIT and the batch interpreter."""
    if engine == "table":
        monkeypatch.setenv("MIMIC_SPREAD_OWN", "0")
        _check(prog, 64, 2999, sched, "spread", spread=1, align=80)
    elif engine == "one_lane":
        _check(prog, 64, 2999, sched, "jit", spread=0, align=80)
    else:
        _check(prog, 64, 2999, sched, "interp", exec_mode="interp", align=80)


def test_from_numpy_on_the_device_is_uniform(gpu):
    buf, off, lens = W.make_packets(512, align=128)
    b = M.XDPBatch.from_numpy(buf, off, lens, device="cuda:0", ingress=1, schedule=M.SCHED_INTERLEAVED)
    assert b.pkt_off is None and b.pkt_len is None and (b.pkt_stride, b.pkt_len_all) == (128, 64)
    assert b.packet_bytes(3) == bytes(buf[3 * 128:3 * 128 + 64])


# ---------------------------------------------------------------------------------------------
# mimic_run_xdp_many: the forms of the batches of one owned launch
# ---------------------------------------------------------------------------------------------
MANY = {
    "all_uniform_1": [("u", 64)],
    "all_uniform_2": [("u", 64)] * 2,
    "all_uniform_8": [("u", 64)] * 8,
    "all_arrays_1": [("a", 64)],
    "all_arrays_2": [("a", 64)] * 2,
    "all_arrays_8": [("a", 64)] * 8,
    "alternating_8": [("u", 64), ("a", 64)] * 4,
    "alternating_from_arrays": [("a", 64), ("u", 64), ("a", 128), ("u", 128)],
    "strides_differ": [("u", 64), ("u", 128), ("u", 80), ("u", 200), ("o", 64), ("l", 128)],
}


@pytest.mark.parametrize("prog", list(PROGS))
@pytest.mark.parametrize("sched", ["interleaved", "chunked"])
@pytest.mark.parametrize("case", list(MANY))
def test_many(gpu, prog, sched, case):
    """K = 1, 2 and 8; every batch uniform, every batch with arrays, the two alternating (the batch
    boundary's prefetch crosses forms both ways), and strides that differ within one launch
    ('o': offsets dropped only, over varying lengths; 'l': lengths dropped only, shuffled slots)."""
    V, n = 64, 64 * 4 + 13
    sc = _sc(PROGS[prog](), V)
    mode = M.SCHED_INTERLEAVED if sched == "interleaved" else M.SCHED_CHUNKED
    cpu = W.schedule_cpu(n, V, sched)
    ovm, omids, opids = build_oracle(sc)
    vm, maps, pids = build_engine(sc)
    dev, want = [], []
    for k, (form, align) in enumerate(MANY[case]):
        sizes = dict(sizes=(64, 40, 20), weights=(4, 1, 1)) if form == "o" else {}
        buf, off, lens = W.make_packets(n, seed=100 + k, align=align, **sizes)
        if form == "l":
            off = off[np.random.default_rng(k).permutation(n)].copy()
        b = buf.copy()
        o = ovm.run_xdp_batch(opids[0], b, off, lens, cpu, 0, 0, 1, 0, 0)
        o["pkt"] = b
        want.append(o)
        dev.append(_batch(buf, off, lens, form in "uo", form in "ul", mode))
    res = vm.RunXDPMany(pids[0], dev)
    assert vm.LastExec() == "spread_own"
    for k, (o, r, d) in enumerate(zip(want, res, dev)):
        e = r.numpy(n)
        for f in ("r0", "status", "steps", "err_pc"):
            a, b = np.asarray(o[f]).astype(np.int64), np.asarray(e[f]).astype(np.int64)
            bad = np.nonzero(a != b)[0]
            assert len(bad) == 0, f"batch {k} {f} differs at {bad[:6]}"
        assert np.array_equal(o["pkt"], d.pkt_data.cpu().numpy()), f"batch {k} packet memory"
    for m in sc.maps:
        for c in range(ncpus(sc, m)):
            assert maps[m["name"]].Values(c) == ovm.map_values(omids[m["name"]], c), f"map {m['name']} cpu {c}"
    ovm.close()
    vm.close()


# ---------------------------------------------------------------------------------------------
# validation: no pkt_off and a zero stride would put every packet at the same address
# ---------------------------------------------------------------------------------------------
def test_zero_stride_is_einval(gpu):
    sc = _sc(W.prog_classifier(), 64)
    vm, maps, pids = build_engine(sc)
    buf, off, lens = W.make_packets(256)
    good = _batch(buf, off, lens, True, True, M.SCHED_INTERLEAVED)
    bad = _batch(buf, off, lens, True, True, M.SCHED_INTERLEAVED)
    bad.pkt_stride = 0
    one = _batch(buf[:64], off[:1], lens[:1], True, True, M.SCHED_INTERLEAVED)
    one.pkt_stride = 0
    with pytest.raises(M.MimicError, match="pkt_stride 0"):
        vm.RunXDPBatch(pids[0], bad)
    vm.RunXDPBatch(pids[0], one)          # n = 1: no stride needed
    with pytest.raises(M.MimicError, match="batch 2"):
        vm.RunXDPMany(pids[0], [good, good, bad, good])
    # nothing of the refused call ran: the counters hold the one packet only
    total = sum(int(np.frombuffer(maps["verdicts"].Values(c), np.uint64).sum()) for c in range(64))
    assert total == 1
    # the raw ABI: the same through the struct, as the only batch and as a later one
    lib = _lib.load()
    arr = (_lib.XDPBatch * 2)()
    C.memmove(C.byref(arr, 0), good._c(), C.sizeof(_lib.XDPBatch))
    C.memmove(C.byref(arr, C.sizeof(_lib.XDPBatch)), bad._c(), C.sizeof(_lib.XDPBatch))
    rs = (_lib.XDPResults * 2)()
    assert lib.mimic_run_xdp_many(vm.h, pids[0], arr, rs, 2, None) == -1   # MIMIC_EINVAL
    assert lib.mimic_run_xdp(vm.h, pids[0], C.byref(arr[1]), C.byref(rs[0]), None) == -1
    vm.close()
