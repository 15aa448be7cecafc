"""The address-matrix corpus (tests/memmatrix.py) on the CPU: the oracle equals the model for every
program and every packet, the corpus keeps the shape the GPU module relies on -- every edge offset in
every batch, surviving and failing packets in every aligned group of 64 (the 64 lanes of a wave),
every error status a region's neighbourhood can produce, no store whose bytes nothing reads back --
and the generated source takes the paths the module is about: the lane-varying stack and xdp_md
accesses through cold_load / cold_store, the read-backs after them on the inline fast paths."""
import re

import numpy as np
import pytest

import memmatrix as MM
from harness import kernel_of, run_sequence_oracle
from mimic_amd import jit as J

CHUNKS = MM.chunks()
FORMS = MM.forms()
IDS = [f"{r}_{op}" for r, op in MM.CHUNK_KEYS]
CHUNK = {key: k for k, key in enumerate(MM.CHUNK_KEYS)}
GROUPS = range(0, MM.N_PACKETS, MM.WAVE)


def test_corpus_shape():
    assert len(FORMS) == 68 == 5 * 12 + 2 * 4 and len({f.name for f in FORMS}) == 68
    assert len(CHUNKS) == 17 and all(len(c[1]) == 4 and [f.n for f in c[1]] == [1, 2, 4, 8] for c in CHUNKS)
    assert MM.N_PACKETS == 4 * MM.V_CPUS and MM.V_CPUS % MM.WAVE == 0
    picks = MM.one_per_region_op()
    assert len(picks) == 17 and len({(FORMS[k].region, FORMS[k].op) for k in picks}) == 17
    assert {FORMS[k].n for k in picks} == set(MM.SIZES)
    assert sum(f.rooms for f in FORMS) == 4 and all(f.region == "packet" for f in FORMS if f.rooms)
    for k in range(len(FORMS)):
        b = MM.batch(k)
        assert (b["cpu"] == np.arange(MM.N_PACKETS) % MM.V_CPUS).all()          # test_opmatrix_cpu: lanes = packets
        assert int(b["lens"].min()) >= 16
        if FORMS[k].region == "packet":
            assert int(b["lens"].min()) == 16 and int(b["lens"].max()) == 1514
        if FORMS[k].rooms:
            assert int(b["headroom"].max()) > 16 and int(b["tailroom"].max()) == 16 and int(b["headroom"].min()) == 0
        # a quarter of the odd packets carry bits 32..63
        hi = (b["delta"][1::2] >> np.uint64(32)).astype(np.int64)
        small = b["delta"][1::2].astype(np.int64).astype(np.int32).astype(np.int64)
        n_hi = int(((hi != 0) & (hi != 0xFFFFFFFF)).sum() + ((hi == 0xFFFFFFFF) & (small >= 0)).sum())
        assert 90 <= n_hi <= 170, (FORMS[k].name, n_hi)


def test_stored_values_differ_from_the_prefill_in_every_byte():
    pre = set(MM.PREFILL.to_bytes(8, "little"))
    imm = (MM.ST_IMM & MM.M64).to_bytes(8, "little")
    assert 0 not in imm and not pre & set(imm) and 0 not in pre
    for k in range(len(FORMS)):
        v = MM.batch(k)["value"].view(np.uint8)
        assert int(v.min()) >= 0x81 and int(v.max()) < min(pre)


def test_model_literals():
    """The layout and the access rules by hand, so that the model cannot drift with the oracle."""
    first, fs = CHUNKS[0]                                      # no maps, 4 programs of 9 addresses each
    sp = MM.space_of(fs)
    assert sp.prog_addr[0] == 0x10000 and sp.prog_addr[3] == 0x10000 + 27 and sp.static_next == 0x10000 + 36
    stack, pkt, xdp = sp.new_process(bytes(range(16)), 3, 5, (7, 8, 9))
    St = 0x10024
    assert (stack.addr, pkt.addr, xdp.addr) == (St, St + 2049, St + 2049 + 24 + 1)
    assert bytes(pkt.mem) == bytes(3) + bytes(range(16)) + bytes(5)
    assert [int.from_bytes(xdp.mem[k:k + 4], "little") for k in range(0, 24, 4)] == [pkt.addr + 3, pkt.addr + 19, pkt.addr + 3, 7, 8, 9]
    acc = lambda a, n: sp.access(a, n)[0]
    assert acc(St - 1, 1) == MM.NOT_VMMEM and acc(St, 8) == MM.OK and acc(St + 2040, 8) == MM.OK
    assert acc(St + 2041, 8) == MM.BOUNDS and acc(St + 2047, 1) == MM.OK and acc(St + 2048, 1) == MM.BOUNDS
    assert sp.access(St + 2049, 1)[1] is pkt and acc(pkt.addr + 23, 1) == MM.OK and acc(pkt.addr + 24, 1) == MM.BOUNDS
    assert sp.access(pkt.addr + 25, 4)[1] is xdp and acc(xdp.addr + 20, 4) == MM.OK and acc(xdp.addr + 21, 4) == MM.BOUNDS
    assert acc(xdp.addr + 24, 1) == MM.BOUNDS and acc(xdp.addr + 25, 1) == MM.UNRESOLVED and acc(0xFFFF, 1) == MM.UNRESOLVED
    first, fs = CHUNKS[CHUNK["row24", "stx"]]                  # row24 (V x [object, 24 bytes]) + pad + 4 programs
    sp = MM.space_of(fs)
    row = lambda c: sp.maps["row24"]["values"][c].addr
    assert sp.maps["row24"]["obj"].addr == 0x10000 and row(0) == 0x10000 + 9 + 9 and row(1) == row(0) + 25 + 9
    assert acc(row(0) - 10, 1) == MM.NOT_VMMEM and acc(row(0) - 9, 1) == MM.NOT_DATASEC and acc(row(0) - 1, 1) == MM.NOT_DATASEC
    assert acc(row(1) - 10, 1) == MM.BOUNDS and acc(row(1) - 11, 1) == MM.OK and acc(row(0) + 17, 8) == MM.BOUNDS
    assert sp.maps["pad"]["obj"].addr == row(255) + 25 and sp.prog_addr[0] == row(255) + 25 + 9 + 9
    first, fs = CHUNKS[CHUNK["hsh", "ldx"]]                    # arr (object, 64) + hsh (object, keys 16, values 64)
    sp = MM.space_of(fs)
    arr, hsh = sp.maps["arr"], sp.maps["hsh"]
    assert arr["values"][0].addr == 0x10009 and hsh["obj"].addr == 0x10009 + 65 and hsh["keys"].addr == hsh["obj"].addr + 9
    assert hsh["values"][0].addr == hsh["keys"].addr + 17 and hsh["slots"] == {b"\x11\0\0\0": 0, b"\x22\0\0\0": 1}
    assert acc(hsh["values"][0].addr - 1, 1) == MM.BOUNDS and acc(hsh["values"][0].addr - 2, 1) == MM.OK
    # ST's constant is sign-extended into an 8-byte store; addresses are truncated to 32 bits
    raw = MM.A.assemble([MM.A.st(8, 10, -8, -2), MM.A.ldx(8, 0, 10, -8), MM.A.exit_()])[0]
    assert MM.run_process(sp, MM.decode(raw, [], sp), b"")[:4] == (MM.OK, MM.M64 - 1, 3, -1)
    raw = MM.A.assemble([MM.A.ld_imm64(2, 0xABCD_0000_0000), MM.A.alu64("add", 2, 10, reg=True), MM.A.stx(2, 2, -2, 2),
                         MM.A.ldx(8, 0, 10, -8), MM.A.exit_()])[0]
    s = MM.run_process(sp, MM.decode(raw, [], sp), b"")
    assert s[:4] == (MM.OK, ((sp.static_next + 256) & 0xFFFF) << 48, 6, -1)
    raw = MM.A.assemble([MM.A.mov64_imm(0, 7), MM.A.ldx(1, 3, 10, 2048 - 256), MM.A.exit_()])[0]
    assert MM.run_process(sp, MM.decode(raw, [], sp), b"")[:4] == (MM.BOUNDS, 7, 2, 1)


@pytest.mark.parametrize("c", range(len(CHUNKS)), ids=IDS)
def test_oracle_equals_model(c):
    first, fs = CHUNKS[c]
    outs, maps, _ = run_sequence_oracle(MM.scenario(fs), MM.runs(first, fs))
    want, want_maps = MM.expected(c)
    assert len(outs) == len(fs) == len(want)
    for k, o in enumerate(outs):
        assert len(o["r0"]) == MM.N_PACKETS
        MM.assert_model(first + k, want[k], o, "oracle")
    MM.assert_model_maps(want_maps, maps, "oracle")
    assert set(want_maps) == set(maps)


def test_every_edge_offset_in_every_batch():
    for k, f in enumerate(FORMS):
        b = MM.batch(k)
        n = len(MM.edges(f))
        assert n <= MM.WAVE // 2, "an aligned group of 64 packets walks the whole list"
        assert set(b["edge"][0::2].tolist()) == set(range(n)), f.name
        for j in range(0, MM.N_PACKETS, 2):                     # ... at the offset the list says
            H, T = MM._rooms(b, j)
            base = H if f.region == "packet" else MM.REGION[f.region].base_off
            want = MM.edges(f, H, int(b["lens"][j]), T)[int(b["edge"][j])] - base
            assert int(b["delta"][j].astype(np.int64)) == want
    f = FORMS[[x.name for x in FORMS].index("stack_stx4")]
    W = MM.window_lo()
    assert W == 256 - 8 * MM.lds_q() and {W - 4, W - 3, W - 1, W, 252, 256, 508, 512, 540, 544, 576, 2044, 2045, 2048} <= set(MM.edges(f))
    assert sum((o & 7) + 4 > 8 and W <= o < 256 for o in MM.edges(f)) >= 1      # a straddling access inside the window
    assert sum((o & 7) + 4 > 8 and o > 512 for o in MM.edges(f)) >= 1           # ... and above STK_FINE


@pytest.mark.parametrize("c", range(len(CHUNKS)), ids=IDS)
def test_every_wave_has_survivors_and_every_error(c):
    first, fs = CHUNKS[c]
    want, _ = MM.expected(c)
    for k, f in enumerate(fs):
        st = want[k]["status"]
        have = set(st.tolist())
        assert have >= {MM.OK, *MM.REGION[f.region].statuses}, (f.name, have)
        assert have <= {MM.OK, MM.UNRESOLVED, MM.NOT_VMMEM, MM.BOUNDS, MM.NOT_DATASEC}
        at = f.access_pc
        bad = st != MM.OK
        assert (want[k]["err_pc"][bad] == at).all(), "every failing packet fails in the lane-varying access"
        assert (want[k]["steps"][bad] == at + 1).all() and (want[k]["r0"][bad] != 0).all()
        if f.region not in ("row24", "row72"):                  # (those fold the row first)
            assert (want[k]["r0"][bad] == MM.batch(first + k)["value"][bad]).all()
        assert len(set(want[k]["r0"][~bad].tolist())) > 0.9 * int((~bad).sum())
        for g in GROUPS:
            w = st[g:g + MM.WAVE]
            assert int((w == MM.OK).sum()) >= 8 and int((w != MM.OK).sum()) >= 4, (f.name, g, int((w == MM.OK).sum()))


STORE_CHUNKS = [k for k, (_, op) in enumerate(MM.CHUNK_KEYS) if op != "ldx"]


@pytest.mark.parametrize("c", STORE_CHUNKS, ids=[IDS[k] for k in STORE_CHUNKS])
def test_no_store_is_invisible(c):
    """For every store form and every surviving packet, what the model leaves (R0, packet bytes, the
    vCPU's map bytes) differs from a run with that one store left out."""
    first, fs = CHUNKS[c]
    outs, _ = MM.model_sequence(first, fs, skip_store=True)
    want, _ = MM.expected(c)
    n = 0
    for k, f in enumerate(fs):
        assert (outs[k]["r0"] == want[k]["r0"]).all()           # the counterfactual runs disturb nothing
        if f.op == "ldx":
            continue
        ok = np.nonzero(outs[k]["status"] == MM.OK)[0]
        for j in ok:
            real, skip = outs[k]["real"][j], outs[k]["skip"][j]
            assert real[0] != skip[0], f"{f.name} packet {j}: R0 does not see the store"
            n += 1
    assert n > 300 * 4


def _block(src, pc):
    a = src.index(f"\n    // {pc}: op")
    b = src.index(f"\n    // {pc + 1}: op", a)
    return src[a:b]


def _slots(f):
    """[(slot, Insn)] of a form's program."""
    out, pc = [], 0
    for x in f.items:
        if isinstance(x, str):
            continue
        out.append((pc, x))
        pc += x.slots
    return out


PKT_FAST = re.compile(r"ga_ = \(uint32_t\)\(r9 \+ 0x0ull\);\n\s*if \(\(uint64_t\)\(uint32_t\)\(ga_ - P\) \+ (\d)u <= L\.M\)")


def test_generated_paths():
    """What the JIT generates for these programs (jit.kernel_source, no device)."""
    seen = {}
    for c, (first, fs) in enumerate(CHUNKS):
        src = J.kernel_source(*kernel_of(MM.scenario(fs)))
        assert "L_defer:" in src and "COLD_CALL(cold" not in src, "the chunk kernels defer their slow paths to the resume kernel"
        assert re.search(r"#define MIMIC_LDS_STACK_Q (\d+)", src).group(1) == str(MM.lds_q())
    for k, f in enumerate(FORMS):
        src = J.kernel_source(*kernel_of(MM.scenario([f])))
        assert "COLD_CALL(cold" in src and "L_defer:" not in src, f.name
        assert f"#define MIMIC_LDS_STACK_Q {MM.lds_q()}\n" in src
        blk = _block(src, f.access_pc)
        m = PKT_FAST.search(blk)
        assert m and int(m.group(1)) == f.n, f"{f.name}: the packet fast form comes first"
        cold = "cold_load" if f.op == "ldx" else "cold_store"
        assert f"COLD_CALL({cold}(kp, sp_, ga_, {f.n}u" in blk, f.name
        if f.region in ("stack", "xdp_md"):
            # no inline stack_* / xdp_* for an address the generator cannot place: the cold path
            assert "stack_" not in blk and "xdp_" not in blk, f.name
        form = "vc" if "vc_load(vc0_" in blk or "vc_store(vc0_" in blk else "lvc" if "lvc_" in blk else "t_lo"
        assert "ga_ - L.t_lo" in blk
        seen.setdefault(f.region, set()).add(form)
        # the read-backs after it
        n_stack = n_xdp = n_vc = 0
        for pc, x in _slots(f):
            if pc <= f.access_pc or (x.op & 7) != MM.A.LDX or pc == f.access_pc + 1:
                continue
            b = _block(src, pc)
            if x.src == 10:
                assert "r4 = stack_load(kp, L, ga_ - kp.static_next" in b, (f.name, pc)
                n_stack += 1
            elif x.src == 6:
                assert "xdp_load(" in b and "COLD_CALL" not in b.split("xdp_load(")[0], (f.name, pc)
                n_xdp += 1
            elif x.src == 1:
                n_vc += "vc_load(" in b
        assert n_stack >= 2 and n_xdp >= 2
        if f.region == "stack":
            assert n_stack == len(MM.stack_readback()) == 16
        if f.region in ("row24", "row72") and f.op != "ldx":
            assert n_vc == len(MM.ROW_WORDS[f.region])
    # which form the lane-varying access of each region has beside the packet form and the cold path
    assert seen == {"stack": {"t_lo"}, "packet": {"t_lo"}, "xdp_md": {"t_lo"}, "row24": {"vc"}, "row72": {"lvc"},
                    "arr": {"t_lo"}, "hsh": {"t_lo"}}


def test_proc_cases():
    for k, f in enumerate(FORMS):
        cases = MM.proc_cases(k)
        assert len(cases) == 32 and {c for _, c in cases} == {0, 1, 2, 3}
        n = len(MM.edges(f))
        L = 64 if f.region == "packet" else 16
        for j, e in enumerate(MM.edges(f, 0, L, 0)[:32]):
            d = int.from_bytes(cases[j][0][:4], "little", signed=True)
            assert d == e - MM.REGION[f.region].base_off
        assert n <= 32
        assert sum(int.from_bytes(p[4:8], "little") != 0 for p, _ in cases) == 4
