"""The operand-matrix corpus (tests/opmatrix.py) on the CPU: the oracle equals the model for every
program and every packet, and the corpus keeps the properties the GPU module relies on -- every edge
pair in every batch, every class of shift count / divisor in every aligned group of 64 packets (the
64 lanes of a wave), both outcomes of every jump, panicking packets beside live ones."""
import numpy as np
import pytest

import opmatrix as OM
from harness import run_sequence_oracle
from mimic_amd import asm as A

CHUNKS = OM.chunks()
PAIRS = OM.pairs()
GROUPS = [PAIRS[g:g + OM.WAVE] for g in range(0, OM.N_PACKETS, OM.WAVE)]


def test_corpus_shape():
    assert len(OM.FORMS) == 258 and len(CHUNKS) == 7 and len(CHUNKS) <= 8
    assert len(PAIRS) == OM.N_PACKETS == 4 * OM.V_CPUS and OM.V_CPUS % OM.WAVE == 0
    kinds = {}
    for f in OM.FORMS:
        kinds.setdefault((f.kind, f.cls), []).append(f)
    assert len(kinds[("jmp", "x")]) == 13 and len(kinds[("jmp", "k")]) == len(kinds[("jmp", "k32")]) == 44
    x_alu = [f for f in OM.FORMS if f.kind == "alu" and f.op & A.X and (f.op & 0xF0) != A.END]
    assert len(x_alu) == 24 and len({f.op for f in x_alu}) == 24
    assert len(OM.DIV_X) == 4


def test_lanes_of_a_wave_hold_consecutive_packets():
    """What the explicit schedule does with cpu[k] = k % V (engine.cpp: a stable counting sort by
    vCPU, lane = vCPU; runtime.h pkt_index: the j-th packet of the lane's run): in round j lane g
    runs packet j * V + g, so an aligned group of 64 lanes runs an aligned group of 64 packets."""
    cpu = OM.batch()[3]
    V = OM.V_CPUS
    order = np.argsort(cpu, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(cpu, minlength=V))])
    assert (np.diff(start) == OM.N_PACKETS // V).all()
    for j in range(OM.N_PACKETS // V):
        at_round = order[start[:-1] + j]
        assert (at_round == j * V + np.arange(V)).all()


@pytest.mark.parametrize("c", range(len(CHUNKS)), ids=[f"chunk{k}_{len(c[1])}" for k, c in enumerate(CHUNKS)])
def test_oracle_equals_model(c):
    first, forms = CHUNKS[c]
    outs, _, _ = run_sequence_oracle(OM.scenario(forms), OM.runs(forms))
    assert len(outs) == len(forms)
    for k, o in enumerate(outs):
        assert len(o["r0"]) == OM.N_PACKETS
        OM.assert_model(first + k, o, "oracle")
        assert np.array_equal(o["pkt"], OM.batch()[0]), "no program of the corpus stores"


def test_every_edge_pair_in_every_batch():
    have = set(PAIRS[0::2])
    assert len(OM.EDGES) == len(set(OM.EDGES)) == 22
    assert all((a, b) in have for a in OM.EDGES for b in OM.EDGES)


def test_every_wave_sees_every_count_and_divisor_class():
    classes = (lambda b: b == 0, lambda b: b != 0 and b & OM.M32 == 0, lambda b: 1 <= b <= 31,
               lambda b: 32 <= b <= 63, lambda b: b >= 64)
    assert len(GROUPS) == OM.N_PACKETS // OM.WAVE
    for g, grp in enumerate(GROUPS):
        for k, cl in enumerate(classes):
            assert any(cl(b) for _, b in grp), f"packets {g * OM.WAVE}..: no b of class {k}"


def test_random_pairs_cover_every_quotient_size():
    """The odd packets: a and b of every bit length, so quotients of most of the 65 possible bit
    lengths (a quotient of q bits needs lengths q apart: about 512 (64 - q) / 4096 pairs, under one
    for q > 56) and in both halves of the long division (above and below 32 bits)."""
    odd = PAIRS[1::2]
    assert {a.bit_length() for a, _ in odd} == set(range(1, 65)) == {b.bit_length() for _, b in odd}
    sizes = {(a // b).bit_length() for a, b in odd}
    assert len(sizes) >= 48 and set(range(0, 41)) <= sizes and max(sizes) > 56


def test_register_jumps_see_both_outcomes():
    n = 0
    for k, f in enumerate(OM.FORMS):
        if f.kind != "jmp" or f.cls != "x":
            continue
        r0 = OM.expected(k)["r0"]
        assert (OM.expected(k)["status"] == OM.OK).all()
        assert 0 < int(r0.sum()) < len(r0), f.name
        for g in range(0, OM.N_PACKETS, OM.WAVE):       # and diverge inside every wave
            assert 0 < int(r0[g:g + OM.WAVE].sum()) < OM.WAVE, (f.name, g)
        n += 1
    assert n == 13


def test_immediate_jumps_see_both_outcomes():
    for cls in ("k", "k32"):
        for cond in OM.CONDS:
            both = 0
            for k, f in enumerate(OM.FORMS):
                if f.cls == cls and f.cond == cond:
                    r0 = OM.expected(k)["r0"]
                    both += 0 < int(r0.sum()) < len(r0)
            assert both >= 1, (cls, cond)


def test_division_panics_beside_live_lanes():
    for f in OM.DIV_X:
        st = OM.expected(OM.FORMS.index(f))["status"]
        assert set(st.tolist()) == {OM.OK, OM.DIV0}
        for g in range(0, OM.N_PACKETS, OM.WAVE):
            w = st[g:g + OM.WAVE]
            assert (w == OM.DIV0).any() and (w == OM.OK).any(), (f.name, g)
    # the 32-bit forms panic on more packets: b != 0 with uint32(b) == 0
    n = {f.name: int((OM.expected(OM.FORMS.index(f))["status"] == OM.DIV0).sum()) for f in OM.DIV_X}
    assert n["alu32_div_x"] > n["alu64_div_x"] and n["alu32_mod_x"] > n["alu64_mod_x"]


def test_unsupported_and_panicking_immediates():
    by = {f.name: k for k, f in enumerate(OM.FORMS)}
    for name, status in (("jsgt32_x_no_slot", OM.UNSUP), ("end_alu64_class", OM.UNSUP), ("alu64_arsh_k_ffffffff", OM.SHIFT),
                         ("alu32_arsh_k_ffffffff", OM.SHIFT), ("alu64_div_k_0", OM.DIV0), ("alu32_mod_k_0", OM.DIV0)):
        e = OM.expected(by[name])
        assert (e["status"] == status).all() and (e["r0"] == 0).all()
        at = 4 if OM.FORMS[by[name]].kind == "jmp" else 3
        assert (e["err_pc"] == at).all() and (e["steps"] == at + 1).all()


def test_model_literals():
    """A few values by hand, so that the model cannot drift with the oracle (make_golden.py's
    quirk ledger has the same numbers)."""
    V = 0x1122_3344_AABB_CCDD
    ex = OM.execute
    assert ex(0xD4, 16, V, 0) == (OM.SET, 0xDDCC) and ex(0xDC, 16, V, 0) == (OM.SET, 0xCCDD)
    assert ex(0xD4, 32, V, 0) == (OM.SET, 0xDDCCBBAA) and ex(0xDC, 32, V, 0) == (OM.SET, 0xAABBCCDD)
    assert ex(0xD4, 64, V, 0) == (OM.SET, 0x44332211) and ex(0xDC, 64, V, 0) == (OM.SET, 0x11223344)
    assert ex(0xD4, 8, V, 0) == (OM.SET, V)
    assert ex(0x84, 0, 0x80000000, 0) == (OM.SET, 0xFFFFFFFF80000000)
    assert ex(0x84, 0, 0xABCD_0000_0000_0002, 0) == (OM.SET, 0xFFFFFFFFFFFFFFFE)
    assert ex(0x8F, 0, 7, 3) == (OM.SET, OM.M64 - 6)
    assert ex(0xCC, 0, 0x80000000, 0x1_0000_0001) == (OM.SET, OM.M64)      # count not truncated
    assert ex(0xCC, 0, 0x40000000, 32) == (OM.SET, 0) and ex(0xCF, 0, 1 << 63, 64) == (OM.SET, OM.M64)
    assert ex(0xCF, 0, 1 << 62, 64) == (OM.SET, 0) and ex(0xCF, 0, 1 << 63, 32) == (OM.SET, 0xFFFFFFFF80000000)
    assert ex(0xC7, -1, 1, 0) == (OM.PANIC, OM.SHIFT)
    assert ex(0x6C, 0, 1, 0x1_0000_0001) == (OM.SET, 2) and ex(0x77, -1, OM.M64, 0) == (OM.SET, 0)
    assert ex(0x3C, 0, 9, 0x1_0000_0000) == (OM.PANIC, OM.DIV0) and ex(0x3F, 0, 9, 0x1_0000_0000) == (OM.SET, 0)
    assert ex(0x1D, 0, 0x1_0000_0005, 5) == (OM.JUMP, True)                 # Q1
    assert ex(0x6D, 0, 0x80000000, 1) == (OM.JUMP, False) and ex(0x7D, 0, 0x80000000, 1) == (OM.JUMP, False)
    assert ex(0x15, 5, 0x1_0000_0005, 0) == (OM.JUMP, False) and ex(0x16, 5, 0x1_0000_0005, 0) == (OM.JUMP, True)
    assert ex(0x75, -1, 0, 0) == (OM.JUMP, True) and ex(0x35, -1, 0, 0) == (OM.JUMP, False)
    assert ex(0xB5, -1, OM.M64, 0) == (OM.JUMP, True) and ex(0xB6, -1, 0x1_FFFF_FFFF, 0) == (OM.JUMP, True)
    assert ex(0x45, 1, 1, 0) == (OM.JUMP, False) and ex(0x45, 1, 2, 0) == (OM.JUMP, True)   # Q3
    assert ex(0x4D, 0, 0x1_0000_0000, 0x1_0000_0000) == (OM.JUMP, False)
    assert ex(0x4E, 0, 0x1_0000_0000, 0x1_0000_0000) == (OM.JUMP, True)
    assert ex(0xFF, 0, OM.M64, 0) == (OM.JUMP, True) and ex(0xFF, 0, 5, 3) == (OM.JUMP, False)
    assert ex(0x6E, 0, 1, 0) == (OM.NOSLOT, OM.UNSUP)


def test_proc_pairs():
    assert len(OM.PROC_PAIRS) == 32 and [p for p in OM.PROC_PAIRS[:22]] == [(v, v) for v in OM.EDGES]
    assert all(b & OM.M32 == 0 for _, b in OM.PROC_PAIRS[22:])
    assert sum(b == 0 for _, b in OM.PROC_PAIRS[22:]) == 5
