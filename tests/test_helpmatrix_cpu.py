"""The helper-matrix corpus (tests/helpmatrix.py) on the CPU: the oracle equals the model for every
program and every packet, the corpus keeps the shape the GPU module relies on -- every edge in every
batch, surviving and failing packets (or two continuations) in every aligned group of 64 (the 64 lanes
of a wave), every status and errno a form can produce, no update nothing reads back, no two vCPUs on
one key of a shared map -- and the generated source takes the paths the module is about: the inline
lookup / tail-call forms ahead of the cold call where the map is an LD_IMM64 of the call's block, the
cold call alone where the map pointer comes from the packet."""
import collections

import numpy as np
import pytest

import helpmatrix as HM
from harness import kernel_of, run_sequence_oracle
from mimic_amd import jit as J

A = HM.A
CHUNKS = HM.chunks()
FORMS = HM.forms()
IDS = [f"{first:02d}_{fs[0].name}" for first, fs in CHUNKS]
ONE = HM.one_per_group()
GROUPS = range(0, HM.N_PACKETS, HM.WAVE)


def test_corpus_shape():
    assert len(FORMS) == 34 and len({f.name for f in FORMS}) == 34
    assert [len(fs) for _, fs in CHUNKS] == [4] * 8 + [2]
    assert collections.Counter(f.group for f in FORMS) == {1: 3, 2: 19, 3: 5, 4: 5, 5: 1, 6: 1}
    assert [FORMS[k].group for k in ONE] == [1, 2, 3, 4, 5, 6]
    assert HM.N_PACKETS == 4 * HM.V_CPUS and HM.V_CPUS % HM.WAVE == 0
    types = collections.Counter(m["type"] for m in HM.MAPS)
    assert types == {2: 2, 6: 2, 1: 2, 5: 1, 3: 1}
    rows = sorted(m["max_entries"] * m["value_size"] for m in HM.MAPS if m["type"] == 6)
    assert rows == [24, 72] and any(m["value_size"] % 8 for m in HM.MAPS)
    keys = sorted(m["key_size"] for m in HM.MAPS if m["type"] == 1)
    assert keys == [20, 40]                                    # the inline probe takes keys up to 32 bytes
    # the forms that insert into or delete from a shared hash map from many vCPUs share a VM with no form that names a
    # hash map otherwise (the plain array's index update may stand beside them: it folds an array address only)
    for _, fs in CHUNKS:
        if any(f.mutates_hash for f in fs):
            assert all(f.mutates_hash or f.name == "idx_arrv_update" for f in fs)
    assert sum(f.rooms for f in FORMS) == 3
    for first, fs in CHUNKS:
        for j, f in enumerate(fs):
            b = HM.batch_for(tuple(fs), j)
            assert (b["cpu"] == np.arange(HM.N_PACKETS) % HM.V_CPUS).all()          # test_opmatrix_cpu: lanes = packets
            assert int(b["lens"].min()) >= 16
            if f.rooms:
                assert int(b["headroom"].max()) > 16 and int(b["tailroom"].max()) == 16 and int(b["headroom"].min()) == 0
            if f.kind == "adjtail":
                assert int((b["lens"] == 20).sum()) >= HM.N_PACKETS // 2
            # a quarter of the odd packets carry random bits 32..63 on top of the delta
            d = b["delta"][1::2]
            hi = (d >> np.uint64(32)).astype(np.int64)
            neg = d.astype(np.int64).astype(np.int32).astype(np.int64) < 0
            n_hi = int(((hi != 0) & ~((hi == 0xFFFFFFFF) & neg)).sum())
            assert 90 <= n_hi <= 170 or f.mutates_hash and f.kind == "key" and n_hi == 512, (f.name, n_hi)


def test_model_literals():
    """The layout and the helpers by hand, so that the model cannot drift with the oracle."""
    fs = CHUNKS[0][1]
    sp = HM.space_of(fs)
    obj = lambda n: sp.maps[n]["obj"].addr          # noqa: E731
    val = lambda n, c=0: sp.maps[n]["values"][c].addr   # noqa: E731
    # arr: object 8 + values 72; pc24: object, 256 x (object 8, values 24); pc72: object, 256 x (8, 72)
    assert obj("arr") == 0x10000 and val("arr") == 0x10009 and obj("pc24") == 0x10009 + 73
    assert val("pc24", 0) == obj("pc24") + 9 + 9 and val("pc24", 1) == val("pc24", 0) + 25 + 9
    assert obj("pc72") == val("pc24", 255) + 25 and val("pc72", 2) == obj("pc72") + 9 + 9 + 2 * (73 + 9)
    # h20: object, keys 4096 * 20, values 4096 * 12; ph: 256 values backings of 2048 * 12, the object, the keys
    assert sp.maps["h20"]["keys"].addr == obj("h20") + 9 and val("h20") == obj("h20") + 9 + 4096 * 20 + 1
    assert val("ph", 1) == val("ph", 0) + 2048 * 12 + 1 and obj("ph") == val("ph", 255) + 2048 * 12 + 1
    assert sp.maps["ph"]["keys"].addr == obj("ph") + 9 and obj("progs") == obj("ph") + 9 + 2048 * 8 + 1
    assert obj("arrv") == val("progs") + 41 and val("arrv") == obj("arrv") + 9
    assert sp.prog_addr[0] == val("arrv") + 1024 * 12 + 1 and sp.static_next == sp.prog_addr[6] + 9
    sp.new_process(bytes(24), 0, 0)
    St = sp.static_next
    # regToMap: a map object's nine addresses, a sub-array object (that CPU's array), double pointers
    name = lambda a: (lambda m: m and (m[0]["spec"]["name"], m[1]))(sp.reg_to_map(a))   # noqa: E731
    assert name(obj("h20")) == name(obj("h20") + 8) == ("h20", -1) and name(obj("h20") + 9) is None    # the keys' first word: 0
    assert name(val("pc72", 5) - 9) == name(val("pc72", 5) - 1) == ("pc72", 5) and name(val("pc72", 5) - 10) is None
    assert name(val("arr")) == ("h20", -1) and name(val("arr") + 12) == ("progs", -1) and name(val("arr") + 24) is None
    assert name(val("arr") + 36) is None and name(val("arr") + 69) is None and name(val("arr") + 1) is None
    assert name(sp.prog_addr[4]) is None and name(0) is None and name((7 << 32) + obj("ph")) == ("ph", -1)
    sp.proc[0].mem[100:104] = obj("h40").to_bytes(4, "little")
    assert name(St + 100) == ("h40", -1) and name(St + 2045) is None and name(St + 2048) is None
    # the keys: readable to the inclusive end's last whole key
    assert sp.read(St + 2048 - 20, 20) == bytes(20) and sp.read(St + 2048 - 19, 20) is None and sp.read(St - 1, 4) is None
    assert sp.read(obj("arr"), 4) is None and sp.read(obj("h20"), 4) is None and sp.read(val("arr") + 68, 4) == HM._init_bytes(5, 12)[8:]
    progs = HM.decoded(fs, sp)

    def run(items, pkt=bytes(24), cpu=0):
        raw, rel = A.assemble(items + [A.exit_()])
        return HM.run_process(sp, progs + [HM.MM.decode(raw, rel, sp)], len(progs), pkt, 0, 0, cpu)[:4]

    key = lambda k: [A.st(4, 10, -4, k), A.mov64_reg(2, 10), A.alu64("add", 2, -4)]     # noqa: E731
    n = lambda it: len(A.assemble(it + [A.exit_()])[0]) // 8                            # noqa: E731
    it = key(5) + [A.ld_map_fd(1, "arr"), A.call(1)]
    assert run(it) == (0, val("arr") + 60, n(it), -1)
    it = key(6) + [A.ld_map_fd(1, "arr"), A.call(1)]
    assert run(it) == (0, 0, n(it), -1)
    it = key(1) + [A.ld_map_fd(1, "pc72"), A.call(1)]
    assert run(it, cpu=3) == (0, val("pc72", 3) + 12, n(it), -1)
    it = key(1) + [A.ld_map_fd(1, "pc72"), A.alu64("add", 1, 9 + 7 * 82 + 4), A.call(1)]       # cpu 7's sub-array object
    assert run(it, cpu=3) == (0, val("pc72", 7) + 12, n(it), -1)
    it = key(6) + [A.mov64_reg(3, 10), A.alu64("add", 3, -16), A.ld_map_fd(1, "pc72"), A.call(2)]
    assert run(it) == (0, 7, n(it), -1)                        # E2BIG, positive
    it = key(0) + [A.mov64_reg(3, 10), A.alu64("add", 3, 2048 - 256 - 23), A.ld_map_fd(1, "pc24"), A.call(2)]
    assert run(it) == (HM.VALUE, 0, n(it) - 1, n(it) - 2)      # 24 bytes from 23 before the stack's end
    it = key(0) + [A.ld_map_fd(1, "pc24"), A.call(3)]
    assert run(it) == (HM.MAP_OP, 0, n(it) - 1, n(it) - 2)
    it = [A.mov64_imm(2, 3), A.ld_map_fd(1, "pc24"), A.call(3)]                              # ... before the key is read
    assert run(it) == (HM.MAP_OP, 0, n(it) - 1, n(it) - 2)
    # an overlapping update is a memmove (the reference copies the value out first): row bytes 1 .. 16 = 01 .. 10, then
    # bytes 4 .. 15 to entry 0 (0 .. 11), and bytes 8 .. 19 to entry 1 (12 .. 23): a forward copy in words would read
    # bytes 16 .. 19 after it wrote them
    fill = [A.ld_map_fd(1, "pc72")] + key(0) + [A.call(1), A.mov64_reg(6, 0), A.ld_imm64(3, 0x0807060504030201), A.stx(8, 6, 0, 3),
                                                  A.ld_imm64(3, 0x100F0E0D0C0B0A09), A.stx(8, 6, 8, 3)]
    it = fill + [A.mov64_reg(3, 6), A.alu64("add", 3, 4)] + key(0) + [A.ld_map_fd(1, "pc72"), A.call(2), A.ldx(8, 0, 6, 0)]
    assert run(it)[:2] == (0, 0x0C0B0A0908070605)
    it = fill + [A.mov64_reg(3, 6), A.alu64("add", 3, 8)] + key(1) + [A.ld_map_fd(1, "pc72"), A.call(2), A.ldx(4, 0, 6, 20)]
    assert run(it, cpu=9)[:2] == (0, 0)
    assert run(it[:-1] + [A.ldx(8, 0, 6, 12)], cpu=9)[:2] == (0, 0x100F0E0D0C0B0A09)
    # hash: FIFO freelist, delete to the tail, absent delete is nil
    h40 = sp.maps["h40"]
    assert h40["slots"] == {HM.PAT: 0, bytes(40): 1} and list(h40["free"]) == [2, 3, 4, 5, 6, 7]
    assert sp.delete(h40, HM.PAT, 0) == 0 and sp.delete(h40, b"x" * 40, 0) == 0 and list(h40["free"])[-1] == 0
    assert sp.update(h40, -1, b"y" * 40, bytes(16), 0) == 0 and h40["slots"][b"y" * 40] == 2
    assert sp.lookup(h40, -1, b"y" * 40, 9) == val("h40") + 32 and sp.lookup(h40, -1, HM.PAT, 0) == 0
    ph = sp.maps["ph"]
    assert sp.lookup(ph, -1, HM.PAT[:8], 200) == val("ph", 200) and sp.update(ph, -1, b"k" * 8, b"v" * 12, 9) == 0
    assert sp.lookup(ph, -1, b"k" * 8, 4) == val("ph", 4) + 12 and bytes(ph["values"][9].mem[12:24]) == b"v" * 12
    assert bytes(ph["values"][4].mem[12:24]) == bytes(12)
    # tail calls: uint32(R3); the three -EINVAL exits; the budget first; an empty program
    tc = lambda r3, r2="progs": [A.mov64_imm(0, 1), A.ld_map_fd(2, r2), A.ld_imm64(3, r3), A.call(12), A.alu64("add", 0, 1000)]  # noqa: E731
    K = HM.FOLD_K
    assert run(tc(0)) == (0, K + HM.T_CONST[0], 9, -1) and run(tc((1 << 32) + 1)) == (0, K + HM.T_CONST[1], 9, -1)
    assert run(tc(9))[:2] == (0, K + HM.T_CONST[1]) and run(tc(2)) == (HM.PC_OOB, 1, 6, 5)
    # slot 3 holds 0, 4 the first target's inclusive end, 5 the byte past the last program, 6 a map object, 7 nothing
    for r3 in (3, 4, 5, 6, 7, 10, 1 << 31):
        want = (0, K + HM.T_CONST[0], 9, -1) if r3 == 4 else (0, (HM.EINVAL + 1000) & HM.M64, 8, -1)
        assert run(tc(r3)) == want, r3
    assert run(tc(0, "arr")) == (HM.TAILCALL, 1, 6, 5) and run(tc(0, "h20")) == (HM.TAILCALL, 1, 6, 5)
    it = [A.mov64_imm(0, 1), A.mov64_imm(2, 5), A.mov64_imm(3, 0), A.call(12)]
    assert run(it) == (HM.MAP_PTR, 1, 4, 3)
    # adjust_tail: -EINVAL for everything but a 20-byte PlainMemory
    adj = lambda: [A.mov64_imm(0, 1), A.mov64_imm(2, -4), A.call(65)]            # noqa: E731
    assert run(adj()) == (0, HM.EINVAL, 4, -1)
    ad2 = [A.ldx(4, 1, 1, 0)] + adj()
    assert run(ad2, pkt=bytes(20)) == (HM.ENGINE_HELPER, 1, 4, 3) and run(ad2, pkt=bytes(21)) == (0, HM.EINVAL, 5, -1)
    assert run([A.call(8)], cpu=77) == (0, 77, 2, -1)


@pytest.mark.parametrize("c", range(len(CHUNKS)), ids=IDS)
def test_oracle_equals_model(c):
    first, fs = CHUNKS[c]
    outs, maps, hashes = run_sequence_oracle(HM.scenario(fs), HM.runs(fs))
    want, want_maps, want_hashes = HM.expected(c)
    assert len(outs) == len(fs) == len(want)
    for k, o in enumerate(outs):
        assert len(o["r0"]) == HM.N_PACKETS
        HM.assert_model(fs, k, want[k], o, "oracle")
    # through the oracle, which is sequential, the hash maps are exact to the slot in every VM
    HM.assert_model_maps([], want_maps, want_hashes, maps, hashes, "oracle")
    assert set(want_maps) == set(maps)


@pytest.mark.parametrize("k", ONE, ids=[FORMS[k].name for k in ONE])
def test_oracle_equals_model_one_program(k):
    fs = [FORMS[k]]
    outs, maps, hashes = run_sequence_oracle(HM.scenario(fs), HM.runs(fs))
    want, want_maps, want_hashes = HM.model_sequence(fs)
    HM.assert_model(fs, 0, want[0], outs[0], "oracle")
    HM.assert_model_maps([], want_maps, want_hashes, maps, hashes, "oracle")
    assert set(want[0]["status"].tolist()) >= {HM.OK, *FORMS[k].statuses}


def test_every_edge_in_every_batch():
    for first, fs in CHUNKS:
        sp = HM._layout(tuple(fs))
        for j, f in enumerate(fs):
            b = HM.batch_for(tuple(fs), j)
            n = len(HM.edges(f, sp, HM._lay(sp, 0, 64, 0), 0))
            assert n <= HM.N_PACKETS // 8, "every edge at least four times in a batch"
            assert set(b["edge"][0::2].tolist()) == set(range(n)) and (b["edge"][1::2] == -1).all(), f.name
            for k in range(0, HM.N_PACKETS, 2):                 # ... at the delta the list says
                H, T = HM.MM._rooms(b, k)
                d, hi = HM.edges(f, sp, HM._lay(sp, H, int(b["lens"][k]), T), k % HM.V_CPUS)[int(b["edge"][k])]
                if f.mutates_hash and f.kind == "key":          # bits 32..47 hold the vCPU + 1 (helpmatrix.make_packet)
                    v = (int(b["delta"][k]) - d) & HM.M64
                    assert v & HM.M32 == 0 and (v >> 32) & 0xFFFF == k % HM.V_CPUS + 1, (f.name, k)
                    continue
                assert int(b["delta"][k]) == (d + (hi << 32)) & HM.M64, (f.name, k)
    # the list's inclusive ends, by hand, for one form of each pointer kind
    sp = HM._layout(tuple(CHUNKS[0][1]))
    lay = HM._lay(sp, 0, 64, 0)
    e = HM.edges(FORMS[0], sp, lay, 3)
    pc72 = sp.maps["pc72"]["values"]
    for a in (0x10008, 0x10009, pc72[3].addr - 9, pc72[3].addr - 1, pc72[3].addr, pc72[4].addr - 9, pc72[255].addr - 1,
              lay["St"] + 256 - 48, lay["P"] + 16, lay["X"], lay["X"] + 25, sp.prog_addr[4] + 8):
        assert (a - 0x10000, 0) in e, hex(a)
    f = FORMS[[x.name for x in FORMS].index("key_stack_h20_lookup")]
    assert {(o - 256, 0) for o in (-1, 0, 1, 2028, 2029, 2047, 2048, 2049, 216)} <= set(HM.edges(f, sp, lay, 0))
    f = FORMS[[x.name for x in FORMS].index("val_own_pc72_update")]
    assert {(o, 0) for o in list(range(13, 36)) + [60, 61, 72, 73, -1]} <= set(HM.edges(f, sp, lay, 0))
    f = FORMS[[x.name for x in FORMS].index("idx_progs_tail")]
    # (d, hi): R3 = (s64)d + (hi << 32), so 2^31 is (-2^31, 1), 2^32 - 1 is (-1, 1) and 2^32 + 1 is (1, 1)
    assert {(0, 0), (9, 0), (10, 0), (11, 0), (-(1 << 31), 1), (-1, 1), (1, 1), (10, 1)} <= set(HM.edges(f, sp, lay, 0))


FAMILY = {2: "array", 3: "array", 6: "percpu_array", 1: "hash", 5: "percpu_hash"}


@pytest.mark.parametrize("c", range(len(CHUNKS)), ids=IDS)
def test_every_wave_has_survivors_failures_and_every_outcome(c):
    first, fs = CHUNKS[c]
    want, _, _ = HM.expected(c)
    for k, f in enumerate(fs):
        st, out = want[k]["status"], want[k]["outcome"]
        have = set(st.tolist())
        assert have == {HM.OK, *f.statuses}, (f.name, have)
        rets = {o for o in out if o is not None and 0 <= o < (1 << 64)}
        assert rets >= set(f.errnos), (f.name, f.errnos)
        bad = st != HM.OK
        at = f.call_pc
        assert (want[k]["err_pc"][bad] == at).all(), "every failing packet fails in the lane-varying call"
        assert (want[k]["r0"][bad] != 0).all()
        if f.kind not in ("budget", "idx"):
            assert (want[k]["steps"][bad] == at + 1).all()
            b = HM.batch_for(tuple(fs), k)
            val = np.array([int.from_bytes(bytes(b["buf"][int(o) + h + 8:int(o) + h + 16]), "little")
                            for o, h in zip(b["off"], np.broadcast_to(b["headroom"], (HM.N_PACKETS,)))], np.uint64)
            assert (want[k]["r0"][bad] == val[bad]).all(), "a failing call leaves R0 as it was"
        assert len(set(want[k]["r0"][~bad].tolist())) > 0.9 * int((~bad).sum())
        if f.kind != "budget":                                  # (a count of 0 exits before it)
            assert all(o is not None for o in out), "every packet reaches the call"
        for g in GROUPS:
            w = st[g:g + HM.WAVE]
            if f.group in (4, 5):                               # nothing (or little) fails: two continuations
                conts = {("hit" if f.op == "lookup" and o > 0 else o) for o in out[g:g + HM.WAVE]}
                assert len(conts) >= 2, (f.name, g, conts)
                if f.kind == "idx" and f.op == "tail":
                    assert len({int(p) for p in want[k]["prog"][g:g + HM.WAVE]}) >= 2, (f.name, g)
                continue
            assert int((w == HM.OK).sum()) >= 8 and int((w != HM.OK).sum()) >= 4, (f.name, g, int((w == HM.OK).sum()))
            if f.name == "mapptr_lookup":                       # three families, two key sizes among the survivors
                named = {m for m, s in zip(want[k]["map"][g:g + HM.WAVE], w) if s == HM.OK}
                assert len({FAMILY[HM.SPEC[m]["type"]] for m in named}) >= 3, (g, named)
                assert len({HM.SPEC[m]["key_size"] for m in named}) >= 2, (g, named)
    if c == 0:      # form 1 names every map, through objects, sub-array objects and double pointers
        ok = want[0]["status"] == HM.OK
        assert {m for m, s in zip(want[0]["map"], ok) if s} == set(HM.SPEC)


UPDATES = [c for c, (_, fs) in enumerate(CHUNKS) if any(f.op == "update" and not f.mutates_hash for f in fs)]


@pytest.mark.parametrize("c", UPDATES, ids=[IDS[c] for c in UPDATES])
def test_no_update_is_invisible(c):
    """For every update form and every surviving packet, R0 differs from a run with that one call
    left out."""
    first, fs = CHUNKS[c]
    outs, _, _ = HM.model_sequence(fs, skip_call=True)
    want, _, _ = HM.expected(c)
    n = 0
    for k, f in enumerate(fs):
        assert (outs[k]["r0"] == want[k]["r0"]).all()           # the counterfactual runs disturb nothing
        if f.op != "update":
            continue
        ok = outs[k]["status"] == HM.OK
        assert (outs[k]["r0"][ok] != outs[k]["skip_r0"][ok]).all(), f"{f.name}: R0 does not see the update"
        n += int(ok.sum())
    assert n > 400


def test_concurrency_conditions():
    """On the model alone: in a mutating form no two vCPUs touch the same key of a shared hash map or
    the same entry of the plain array; no hash map gets half full; a form that inserts into a shared
    hash map folds no hash address."""
    for c, (first, fs) in enumerate(CHUNKS):
        if not any(f.mutating for f in fs):
            continue
        outs, _, _ = HM.model_sequence(fs, log=True)
        want, _, _ = HM.expected(c)
        for k, f in enumerate(fs):
            assert (outs[k]["r0"] == want[k]["r0"]).all()
            if not f.mutating:
                continue
            who = collections.defaultdict(set)
            for name, key, cpu in outs[k]["log"]:
                who[name, key].add(cpu)
            shared = [x for x, cpus in who.items() if len(cpus) > 1]
            assert not shared, (f.name, shared[:4])
            assert outs[k]["fill"] < 0.5, (f.name, outs[k]["fill"])
            if f.mutates_hash:
                if f.kind == "mapptr":                          # the hash maps its lanes name, a key per vCPU
                    assert len(who) > 300 and {n for n, _ in who} == {"h20", "h40", "ph"}
                    # the lanes of one call that free a slot name ONE table: only h20 ever held the form's keys
                    sp = HM.space_of(fs)
                    held = {n for n in ("h20", "h40", "ph") for key in sp.maps[n]["slots"] if key[2:4] == b"\xa2\xc3"}
                    assert held == {"h20"}
                else:
                    assert len(who) > 600 and {n for n, _ in who} == {f.map}
                ins = HM.MM.decode(f.raw, f.relocs, HM._layout(tuple(fs)))
                calls = [pc for pc, x in enumerate(ins) if x[0] == 0x85 and x[4] == A.FN_MAP_LOOKUP_ELEM]
                assert calls
                for pc in calls:                                # r9 = r0; r0 = r8; r7 = 1; if r9 != 0 ...; r7 = 0; fold r7
                    assert [x[:3] for x in ins[pc + 1:pc + 4]] == [(0xBF, 9, 0), (0xBF, 0, 8), (0xB7, 7, 0)], (f.name, pc)
    # every update names its map by an LD_IMM64 of the call's block: one table for all the lanes that take a slot
    assert all(f.kind != "mapptr" for f in FORMS if f.op == "update")
    # the six-entry plain array is never written; the other one at 4 * cpu + j only (the touch log above has it)
    assert not any(f.mutating and f.map == "arr" for f in FORMS) and any(f.mutating and f.map == "arrv" for f in FORMS)


def _block(src, prog, pc):
    a = src.index(f"\n    // {pc}: op", src.index(f"P{prog}_0:") if prog else 0)
    b = src.index(f"\n    // {pc + 1}: op", a)
    return src[a:b]


def test_generated_paths():
    """What the JIT generates for the lane-varying calls (jit.kernel_source, no device)."""
    for c, (first, fs) in enumerate(CHUNKS):
        src = J.kernel_source(*kernel_of(HM.scenario(fs)))
        if len(fs) == HM.CHUNK:
            assert "L_defer:" in src and "COLD_CALL(cold" not in src, "the chunk kernels defer their slow paths to the resume kernel"
    for k, f in enumerate(FORMS):
        src = J.kernel_source(*kernel_of(HM.scenario([f])))
        assert "COLD_CALL(cold" in src and "L_defer:" not in src, f.name
        blk = _block(src, 0, f.call_pc)
        cold = {"lookup": "cold_lookup", "update": "cold_update", "delete": "cold_delete", "tail": "cold_tailcall",
                "adjust": "cold_adjust_tail"}[f.op]
        assert f"COLD_CALL({cold}(kp, sp_)" in blk, f.name
        fast = [x for x in ("lookup_fast", "hash_lookup_fast(", "tail_fast(") if x in blk]
        if f.group == 1:                                        # the map pointer comes from the packet: the cold call alone
            assert not fast, (f.name, fast)
        elif f.op == "lookup":                                  # array form, then hash form, then the cold call
            assert fast == ["lookup_fast", "hash_lookup_fast("], (f.name, fast)
            assert blk.index("lookup_fast") < blk.index("hash_lookup_fast(") < blk.index("COLD_CALL(cold_lookup"), f.name
        elif f.op == "tail" and f.kind in ("idx", "budget"):
            assert fast == ["tail_fast("] and blk.index("tail_fast(") < blk.index("COLD_CALL("), f.name
        else:
            assert not fast, (f.name, fast)


def test_proc_cases():
    for first, fs in CHUNKS:
        sp = HM._layout(tuple(fs))
        for j, f in enumerate(fs):
            cases = HM.proc_cases(fs, j)
            assert len(cases) == 32 and {c for _, c in cases} == {0, 1, 2, 3}
            for n, (pkt, cpu) in enumerate(cases):
                e = HM.edges(f, sp, HM._lay(sp, 0, len(pkt), 0), cpu)
                if n < len(e):
                    d, hi = e[n]
                    m = 4 if f.mutates_hash and f.kind == "key" else 8
                    assert pkt[:m] == HM.MM.pack(d, hi, 0)[:m], (f.name, n)
