"""The owned spread kernel's packet chain (jit.cpp, spread_own): the next packet's descriptor is taken
ahead of this packet's result stores, a thread's packet index advances by one add and one compare,
and what is uniform for the launch is read once.  Every launch here runs against the oracle on one
VM and one oracle VM, launch after launch: per packet R0 / status / steps / err_pc of every batch,
every packet byte, and the per-CPU counter rows after every launch.

MIMIC_SPREAD_OWN_Q fixes the packets per thread: at these sizes the engine's own choice is 1, which
never runs the prefetch of a following packet."""
import numpy as np
import pytest

from harness import Scenario, build_engine, build_oracle, ncpus, packets_to_buffer, run_oracle, spread_kernel_of
from mimic_amd import asm as A, workloads as W

pytestmark = pytest.mark.gpu


def _sc(p, V):
    return Scenario(vcpus=V, maps=p.maps, progs=[(p.name, p.raw, p.relocs)])


def prog_ifaces():
    """R0 = ingress_ifindex | rx_queue_index << 10 | egress_ifindex << 20 of the xdp_md, counted in
    the per-CPU array at key R0 & 3 (the counter lookup gives the program its owned form)."""
    items = [
        A.mov64_reg(6, 1),
        A.ldx(4, 7, 6, 12),           # ingress_ifindex
        A.ldx(4, 8, 6, 16),           # rx_queue_index
        A.ldx(4, 9, 6, 20),           # egress_ifindex
        A.alu64("lsh", 8, 10),
        A.alu64("or", 7, 8, reg=True),
        A.alu64("lsh", 9, 20),
        A.alu64("or", 7, 9, reg=True),
        A.mov64_reg(8, 7),
        A.alu64("and", 8, 3),
        A.stx(4, 10, -4, 8),
        A.mov64_reg(2, 10),
        A.alu64("add", 2, -4),
        A.ld_map_fd(1, "seen"),
        A.call(A.FN_MAP_LOOKUP_ELEM),
        A.jmp("jeq", 0, 0, 3),
        A.ldx(8, 1, 0, 0),
        A.alu64("add", 1, 1),
        A.stx(8, 0, 0, 1),
        A.mov64_reg(0, 7),
        A.exit_(),
    ]
    raw, rel = A.assemble(items)
    return W.Program("xdp_ifaces", raw, rel, [dict(name="seen", type=6, key_size=4, value_size=8, max_entries=4)])


def jit_kernels():
    return [spread_kernel_of(_sc(W.prog_classifier(), V), own=True) for V in (1024, 1000, 256, 4096)] + \
        [spread_kernel_of(_sc(W.prog_parse5(), 1024), own=True), spread_kernel_of(_sc(prog_ifaces(), 1024), own=True)]


class Pair:
    """One engine VM and one oracle VM of a scenario, run launch by launch."""

    def __init__(self, sc):
        import mimic_amd as M

        self.M, self.sc = M, sc
        self.ovm, self.omids, self.opids = build_oracle(sc)
        self.vm, self.maps, self.pids = build_engine(sc)

    def launch(self, batches, sched, results="all", expect="spread_own", **ctx):
        """batches: [(buf, off, lens)]; ctx: headroom / tailroom / ingress / rxq / egress (scalars, or
        arrays per packet used for every batch).  results: all | r0st | r0."""

        M, sc = self.M, self.sc
        s = M.SCHED_INTERLEAVED if sched == "interleaved" else M.SCHED_CHUNKED
        H, T = ctx.get("headroom", 0), ctx.get("tailroom", 0)
        ing, rxq, egr = ctx.get("ingress", 1), ctx.get("rxq", 0), ctx.get("egress", 0)
        outs = []
        for buf, off, lens in batches:
            b = buf.copy()
            o = self.ovm.run_xdp_batch(self.opids[0], b, off, lens, W.schedule_cpu(len(lens), sc.vcpus, sched), H, T,
                                       *[np.full(len(lens), v, np.int32) if np.isscalar(v) else v for v in (ing, rxq, egr)])
            o["pkt"] = b
            outs.append(o)
        dev = [M.XDPBatch.from_numpy(buf, off, lens, device="cuda:0", headroom=H, tailroom=T, ingress=ing, rxq=rxq, egress=egr,
                                     schedule=s)
               for buf, off, lens in batches]
        res = None
        if results != "all":
            res = [M.XDPResults.empty(len(b[2]), "cuda:0", full=False) for b in batches]
            if results == "r0":
                for r in res:
                    r.status = None
        res = self.vm.RunXDPMany(self.pids[0], dev, res) if len(dev) > 1 else [self.vm.RunXDPBatch(self.pids[0], dev[0], res and res[0])]
        assert self.vm.LastExec() == expect
        fields = {"all": ("r0", "status", "steps", "err_pc"), "r0st": ("r0", "status"), "r0": ("r0",)}[results]
        for k, (o, r, d) in enumerate(zip(outs, res, dev)):
            n = len(batches[k][2])
            for f in fields:
                e = getattr(r, f)[:n].cpu().numpy()
                a, b = np.asarray(o[f]).astype(np.int64), e.astype(np.int64)
                bad = np.nonzero(a != b)[0]
                assert len(bad) == 0, f"batch {k} {f} differs at {bad[:6]}"
            assert np.array_equal(o["pkt"], d.pkt_data.cpu().numpy()), f"batch {k} packet memory"
        for m in sc.maps:
            for c in range(ncpus(sc, m)):
                assert self.maps[m["name"]].Values(c) == self.ovm.map_values(self.omids[m["name"]], c), f"map {m['name']} cpu {c}"

    def close(self):
        self.ovm.close()
        self.vm.close()


def _mixed_frames(n, seed):
    """Frames of 14, 33, 34, 35, 36 and 60 bytes (the 24-byte window at 12 fits or not, the 34-byte
    bounds check passes or not) and a 6-byte one (no Ethernet header: the early loads' cold path)."""
    base, off, lens = W.make_packets(n, seed=seed)
    rng = np.random.default_rng(seed)
    sizes = rng.choice([14, 33, 34, 35, 36, 60, 6], size=n)
    pk = [bytes(base[int(off[i]):int(off[i]) + int(sizes[i])]) for i in range(n)]
    return packets_to_buffer(pk)


@pytest.mark.parametrize("sched", ["interleaved", "chunked"])
@pytest.mark.parametrize("V,n,q", [(1000, 1999, 2), (1024, 4001, 2), (1024, 4001, 4), (1000, 7777, 8), (256, 16383, 8),
                                   (256, 16383, 64), (1000, 1100, 1), (1000, 1100, 2)])
def test_ragged_batches(gpu, monkeypatch, V, n, q, sched):
    """n no multiple of V (threads run out mid-way; at n = 1.1 V most threads of the second packet
    have none: below 2 packets per vCPU the engine does not choose the owned form), 2 to 64 packets
    per vCPU, Q packets per thread, three batches in one launch."""
    monkeypatch.setenv("MIMIC_SPREAD_OWN_Q", str(q))
    pr = Pair(_sc(W.prog_classifier(), V))
    pr.launch([W.make_packets(n, seed=W.SEED + 3 * k) for k in range(3)], sched)
    pr.close()


@pytest.mark.parametrize("nb", [1, 2, 3, 8])
def test_batches_per_launch_twice(gpu, monkeypatch, nb):
    """1, 2, 3 and 8 ragged batches in one launch, the same launch twice on one VM (the counters
    accumulate); the descriptor is carried over every batch boundary."""
    monkeypatch.setenv("MIMIC_SPREAD_OWN_Q", "2")
    pr = Pair(_sc(W.prog_classifier(), 1000))
    batches = [W.make_packets(3001, seed=W.SEED + 11 * k) for k in range(nb)]
    pr.launch(batches, "interleaved")
    pr.launch(batches, "interleaved")
    pr.close()


@pytest.mark.parametrize("results", ["all", "r0st", "r0"])
def test_result_sets(gpu, monkeypatch, results):
    """All four result arrays; r0 + status only (XDPResults.empty(full=False)); r0 only."""
    monkeypatch.setenv("MIMIC_SPREAD_OWN_Q", "4")
    pr = Pair(_sc(W.prog_classifier(), 1024))
    pr.launch([W.make_packets(4001, seed=W.SEED + k) for k in range(2)], "interleaved", results=results)
    pr.close()


@pytest.mark.parametrize("sched", ["interleaved", "chunked"])
def test_rooms_between_plain_launches(gpu, monkeypatch, sched):
    """General-form launches on the VM of plain ones: uniform rooms 8 / 16, then per-packet room
    arrays with the rooms pre-filled non-zero (the zeroing is visible), a plain launch before, between
    and after."""
    monkeypatch.setenv("MIMIC_SPREAD_OWN_Q", "2")
    V, n = 1024, 4001
    pr = Pair(_sc(W.prog_classifier(), V))
    plain = [W.make_packets(n, seed=W.SEED + k) for k in range(2)]
    pr.launch(plain, sched)
    base, off, lens = W.make_packets(n, seed=W.SEED + 5)
    pk = [bytes(base[int(off[i]):int(off[i]) + int(lens[i])]) for i in range(n)]
    buf, roff, rlens = packets_to_buffer(pk, 8, 16)
    pr.launch([(buf, roff, rlens)], sched, headroom=8, tailroom=16)
    pr.launch(plain, sched)
    rng = np.random.default_rng(W.SEED)
    Ha, Ta = rng.integers(0, 20, n).astype(np.uint32), rng.integers(0, 20, n).astype(np.uint32)
    buf, roff, rlens = packets_to_buffer(pk, Ha, Ta)
    for i in range(n):   # rooms pre-filled
        o = int(roff[i])
        buf[o:o + int(Ha[i])] = 0xAB
        buf[o + int(Ha[i]) + int(rlens[i]):o + int(Ha[i]) + int(rlens[i]) + int(Ta[i])] = 0xCD
    pr.launch([(buf, roff, rlens)], sched, headroom=Ha, tailroom=Ta)
    pr.launch(plain, sched)
    pr.close()


def test_mixed_frame_lengths(gpu, monkeypatch):
    monkeypatch.setenv("MIMIC_SPREAD_OWN_Q", "4")
    pr = Pair(_sc(W.prog_classifier(), 1024))
    pr.launch([_mixed_frames(4001, W.SEED + k) for k in range(2)], "interleaved")
    pr.close()


def test_parse5_rows_three_batches(gpu, monkeypatch):
    """parse5's 2 KiB counter rows (16 rows per block) over 3 IMIX batches."""
    monkeypatch.setenv("MIMIC_SPREAD_OWN_Q", "2")
    pr = Pair(_sc(W.prog_parse5(), 1024))
    pr.launch([W.make_packets(16001, **W.IMIX, seed=W.SEED + k) for k in range(3)], "interleaved")
    pr.close()


@pytest.mark.parametrize("sched", ["interleaved", "chunked"])
def test_interface_arrays_between_plain_launches(gpu, monkeypatch, sched):
    """A program that returns the context's ingress / rxq / egress: plain launches with the three as
    scalars (the launch's hoisted values reach R0), and between them a general launch with the three
    as per-packet arrays."""
    monkeypatch.setenv("MIMIC_SPREAD_OWN_Q", "2")
    V, n = 1024, 4001
    pr = Pair(_sc(prog_ifaces(), V))
    plain = [W.make_packets(n, seed=W.SEED + k) for k in range(2)]
    pr.launch(plain, sched, ingress=3, rxq=5, egress=7)
    rng = np.random.default_rng(W.SEED + 1)
    arrs = [rng.integers(0, 1000, n).astype(np.int32) for _ in range(3)]
    pr.launch(plain, sched, ingress=arrs[0], rxq=arrs[1], egress=arrs[2])
    pr.launch(plain, sched, ingress=9, rxq=0, egress=2)
    pr.close()


@pytest.mark.parametrize("sched", ["interleaved", "chunked"])
def test_shards_with_packets_per_thread(gpu, monkeypatch, sched):
    """Two engines owning vCPUs [0, 2048) and [2048, 4096) (VMOptShard: vcpu_begin of the second is not
    0), two packets per thread, 4 packets per vCPU; together one oracle run."""
    import mimic_amd as M

    monkeypatch.setenv("MIMIC_SPREAD_OWN_Q", "2")
    V, n = 4096, 4096 * 4
    sc = _sc(W.prog_classifier(), V)
    buf, off, lens = W.make_packets(n, seed=W.SEED + 9)
    cpu = W.schedule_cpu(n, V, sched)
    o = run_oracle(sc, buf, off, lens, cpu)
    s = M.SCHED_INTERLEAVED if sched == "interleaved" else M.SCHED_CHUNKED
    for r in range(2):
        b0 = 2048 * r
        sel = np.nonzero((cpu >= b0) & (cpu < b0 + 2048))[0]
        vm, maps, pids = build_engine(sc, shard=(b0, 2048))
        batch = M.XDPBatch.from_numpy(buf, off[sel], lens[sel], device="cuda:0", schedule=s)
        e = vm.RunXDPBatch(pids[0], batch).numpy(len(sel))
        assert vm.LastExec() == "spread_own"
        for k in ("r0", "status", "steps", "err_pc"):
            assert np.array_equal(np.asarray(o[k])[sel].astype(np.int64), np.asarray(e[k]).astype(np.int64)), (r, k)
        for c in range(b0, b0 + 2048):
            assert maps["verdicts"].Values(c) == o["maps"]["verdicts"][c], c
        vm.close()


def test_shifted_sub_batches_with_packets_per_thread(gpu, monkeypatch):
    """RunXDPHost's sub-batches continue the interleaved schedule (a non-zero sched_shift in all but the
    first), two packets per thread, ragged."""
    import mimic_amd as M

    monkeypatch.setenv("MIMIC_SPREAD_OWN_Q", "2")
    V, n = 1000, 16001
    sc = _sc(W.prog_classifier(), V)
    buf, off, lens = W.make_packets(n, seed=W.SEED + 13)
    o = run_oracle(sc, buf, off, lens, W.schedule_cpu(n, V, "interleaved"))
    vm, maps, pids = build_engine(sc)
    r0, st = vm.RunXDPHost(pids[0], buf, off, lens, schedule=M.SCHED_INTERLEAVED, chunks=3)
    assert vm.LastExec() == "spread_own"
    assert np.array_equal(np.asarray(o["r0"]).astype(np.uint64), r0)
    assert np.array_equal(np.asarray(o["status"]).astype(np.uint8), st)
    for c in range(V):
        assert maps["verdicts"].Values(c) == o["maps"]["verdicts"][c], c
    vm.close()
