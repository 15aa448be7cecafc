"""Load and store semantics on MI355X with per-lane addresses (tests/memmatrix.py).

Every other memory access of the suite has an address its generator knows: wave-uniform, so a wave
takes one way through resolve(), the stack's validity bits, the xdp_md overlay, the value caches.
Here every program takes the address from the packet and runs over 1 024 packets at V = 256, so the
64 lanes of a wave hold 64 different addresses -- the edge offsets of the region interleaved with
random ones, some with bits 32..63 set -- landing in different entries and failing with different
statuses beside lanes that go on and read everything back.

* interpreter and default JIT, one test per (region, access, engine): one VM with the four sizes'
  programs, one batch per program, against the oracle running the same sequence (R0, status, steps,
  err_pc, packet memory, final map bytes) and against the model's own arrays.  Four programs have more
  slow-path sites than the JIT inlines: these kernels leave through the deferred path, so the resume
  kernel runs the access and everything after it from the DeferRec;
* one form per region as a one-program VM, whose kernel calls its cold paths inline (cold_store
  returns sm0 / sm1 / xdp_dirty through the Spill record to the inline fast paths that follow), and
  the same with MIMIC_JIT_FAST=0;
* Process.Run on the stepping interpreter (MIMIC_PROC_JIT=-1) and on the single-process JIT form
  (MIMIC_PROC_JIT=0): 32 offsets per program, the edge list first, model-exact;
* sk_buff (against the oracle only): LDX / STX through __sk_buff's data pointer plus a lane-varying
  delta, from below the headroom to past the tailroom of IMIX frames.

test_memmatrix_cpu.py holds the oracle to the model and gates the corpus."""
import os

import numpy as np
import pytest

import memmatrix as MM
import mimic_amd as M
from harness import assert_same_sequence, build_engine, kernel_of, run_sequence_engine, run_sequence_oracle
from mimic_amd import jit as J

pytestmark = pytest.mark.gpu

CHUNKS = MM.chunks()
FORMS = MM.forms()
IDS = [f"{r}_{op}" for r, op in MM.CHUNK_KEYS]
# One form per region, accesses and sizes rotating.  One per (region, access) would be 17 kernels with
# inlined cold paths and 17 more without fast paths: hipRTC takes 17 s (stack) to 67 s (the 72-byte row)
# for one of them, more than the rest of the module together.
ONE = [FORMS.index(MM.Form(r, op, n)) for r, op, n in (("stack", "stx", 2), ("packet", "st", 4), ("xdp_md", "stx", 8),
                                                        ("row24", "st", 1), ("row72", "stx", 4), ("arr", "ldx", 2),
                                                        ("hsh", "ldx", 8))]
ONE_IDS = [FORMS[k].name for k in ONE]


def jit_kernels():
    """Per chunk the batch kernel and the single-process form, the one-program kernels, the sk_buff
    kernel (compiled before the session)."""
    out = []
    for _, fs in CHUNKS:
        raws, ctx, vc = kernel_of(MM.scenario(fs))
        out += [(raws, ctx, vc), (raws, ctx | 0x100, vc)]
    out += [kernel_of(MM.scenario([FORMS[k]])) for k in ONE]
    out.append(kernel_of(MM.skb_scenario(), 1))
    return out


_ORACLE = {}


def _oracle(key, sc, runs):
    """The oracle's run of a sequence, computed once for every engine; tests only read it."""
    if key not in _ORACLE:
        _ORACLE[key] = run_sequence_oracle(sc, runs)
    return _ORACLE[key]


def _check(first, fs, want, want_maps, oracle, e, mode, tag):
    for k, out in enumerate(e[0]):
        assert out["last_exec"] == mode, f"{fs[k].name} ran on {out['last_exec']}"
        MM.assert_model(first + k, want[k], out, tag)
    MM.assert_model_maps(want_maps, e[1], tag)
    assert_same_sequence(oracle, e, tag=tag)


@pytest.mark.parametrize("mode", ["interp", "jit"])
@pytest.mark.parametrize("c", range(len(CHUNKS)), ids=IDS)
def test_batches(gpu, c, mode):
    first, fs = CHUNKS[c]
    sc, runs = MM.scenario(fs), MM.runs(first, fs)
    if mode == "jit":
        src = J.kernel_source(*kernel_of(sc))
        assert "L_defer:" in src and "COLD_CALL(cold" not in src, "the chunk kernels defer their slow paths"
    want, want_maps = MM.expected(c)
    e = run_sequence_engine(sc, runs, exec_mode=mode)
    _check(first, fs, want, want_maps, _oracle(("chunk", c), sc, runs), e, mode, f"{IDS[c]} ({mode})")


_ONE_MODEL = {}


def _one(k, mode_tag):
    f = FORMS[k]
    sc, runs = MM.scenario([f]), MM.runs(k, [f])
    if k not in _ONE_MODEL:
        _ONE_MODEL[k] = MM.model_sequence(k, [f])
    want, want_maps = _ONE_MODEL[k]
    e = run_sequence_engine(sc, runs, exec_mode="jit")
    _check(k, [f], want, want_maps, _oracle(("one", k), sc, runs), e, "jit", f"{f.name} ({mode_tag})")


@pytest.mark.parametrize("k", ONE, ids=ONE_IDS)
def test_one_program_cold_calls_inline(gpu, k):
    """A one-program set: the cold paths are called where they stand, and what follows runs in the
    same kernel -- the inline stack_load / xdp_load / value-cache forms with the state cold_store
    handed back."""
    src = J.kernel_source(*kernel_of(MM.scenario([FORMS[k]])))
    assert "COLD_CALL(cold" in src and "L_defer:" not in src and "#define MIMIC_COLD_INLINE 1" in src
    _one(k, "cold calls inline")


def _env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    return old


def _env_back(name, old):
    if old is None:
        del os.environ[name]
    else:
        os.environ[name] = old


@pytest.fixture(scope="module")
def fast_off_kernels(gpu):
    """The knob is read when a kernel is generated, which the session prewarm did without it: the
    MIMIC_JIT_FAST=0 forms of the one-program kernels are compiled here, in parallel."""
    old = _env("MIMIC_JIT_FAST", "0")
    try:
        J.prewarm([kernel_of(MM.scenario([FORMS[k]])) for k in ONE])
    finally:
        _env_back("MIMIC_JIT_FAST", old)


@pytest.mark.parametrize("k", ONE, ids=ONE_IDS)
def test_one_program_fast_paths_off(gpu, fast_off_kernels, k, monkeypatch):
    """MIMIC_JIT_FAST=0: every access through resolve(): a difference that is only there with the fast
    paths on is the generator's, not runtime.h's."""
    monkeypatch.setenv("MIMIC_JIT_FAST", "0")
    src = J.kernel_source(*kernel_of(MM.scenario([FORMS[k]])))
    assert "MIMIC_LDS_STACK_Q" not in src and "ga_ - P" not in src
    _one(k, "MIMIC_JIT_FAST=0")


def _engine(sc, after):
    old = _env("MIMIC_PROC_JIT", str(after))
    try:
        return build_engine(sc)
    finally:
        _env_back("MIMIC_PROC_JIT", old)


@pytest.mark.parametrize("tier", ["interp", "jit"])
@pytest.mark.parametrize("c", range(len(CHUNKS)), ids=IDS)
def test_process_run(gpu, c, tier):
    """One VM per chunk, one process at a time on four vCPUs (rows carry over from process to
    process), closed before the next chunk's VM; the model runs the same processes in order."""
    first, fs = CHUNKS[c]
    sp = MM.space_of(fs)
    vm, _, pids = _engine(MM.scenario(fs), -1 if tier == "interp" else 0)
    try:
        for k, f in enumerate(fs):
            ins = MM.decode(f.raw, f.relocs, sp)
            for n, (pkt, cpu) in enumerate(MM.proc_cases(first + k)):
                p = vm.NewProcess(pids[k], M.LinuxContextXDP(Packet=pkt))
                p.SetCPUID(cpu)
                try:
                    p.Run()
                except M.MimicError:
                    pass
                got = (p.Status, p.Registers.R0, p.Steps, p.ErrPC)
                mem = p.Packet()
                ran = vm.LastExec()
                p.Cleanup()
                want = MM.run_process(sp, ins, pkt, 0, 0, cpu)
                d = int.from_bytes(pkt[:4], "little", signed=True)
                assert got == want[:4], (f"{f.name} ({f.ref}) case {n} delta={d} on {ran}: (status, r0, steps, err_pc) "
                                         f"{got} model {want[:4]}")
                assert bytes(mem) == want[4], f"{f.name} case {n} delta={d} on {ran}: packet memory differs"
                assert ran == tier, f"{f.name}: Run on {ran}"
    finally:
        vm.close()


# ---------------------------------------------------------------------------------------------
# sk_buff: against the oracle only
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["interp", "jit"])
def test_skb_batches(gpu, mode):
    sc, runs = MM.skb_scenario(), MM.skb_runs()
    o = _oracle("skb", sc, runs)
    for f, out in zip(MM.SKB_FORMS, o[0]):       # the corpus reaches the rooms, the frame and both ends' neighbours
        st = np.asarray(out["status"])
        assert (st == 0).sum() > 800 and {3, 5, 26} <= set(st.tolist()), f.name
    e = run_sequence_engine(sc, runs, exec_mode=mode)
    for f, out in zip(MM.SKB_FORMS, e[0]):
        assert out["last_exec"] == mode, f"{f.name} ran on {out['last_exec']}"
    assert_same_sequence(o, e, tag=f"sk_buff ({mode})")


# ---------------------------------------------------------------------------------------------
# the finding, as literal vectors: a 2-byte store into a word that was loaded before and is loaded
# again, at an address the compiler cannot place (data + a packet byte).  ld_n / st_n accessed the
# bytes through types that type-based alias analysis keeps apart, so in a kernel whose slow paths
# leave the packet loop (deferred: no call on the way from the first load to the second) the
# compiler kept the first load's word.  kat_skb.json's store_into_reloaded_word is the same program
# in a chunk whose kernel calls its slow paths, where the reload survived.
# ---------------------------------------------------------------------------------------------
def _reload_prog(skb):
    A = MM.A
    data = A.ldx(4, 2, 1, A.SKB["data"]) if skb else A.ldx(4, 2, 1, 0)
    return A.assemble([data, A.ldx(8, 8, 2, 56), A.ldx(1, 7, 2, 22), A.alu64("add", 7, -1), A.mov64_reg(9, 2),
                       A.alu64("add", 9, 7, reg=True), A.stx(2, 9, 0, 8), A.ldx(8, 0, 2, 56), A.exit_()])[0]


@pytest.mark.parametrize("ctx", ["xdp_md", "sk_buff"])
@pytest.mark.parametrize("mode", ["interp", "jit"])
def test_store_into_reloaded_word(gpu, ctx, mode, monkeypatch):
    """Bytes 56..63 of the frame are 82 .. 89 and byte 22 (the TTL) is 64: the store puts the word's
    low 16 bits at 63 and 64: little endian for xdp_md (the word is 0x8988878685848382: 0x82, 0x83),
    big endian for sk_buff (0x8283848586878889: 0x88, 0x89).  The few-slot kernel is compiled here,
    with its slow paths deferred."""
    from harness import Scenario, packets_to_buffer, skb_packets_to_buffer

    monkeypatch.setenv("MIMIC_JIT_COLD", "defer")
    skb = ctx == "sk_buff"
    sc = Scenario(vcpus=1, progs=[("p", _reload_prog(skb), [])])
    src = J.kernel_source(*kernel_of(sc, 1 if skb else 0))
    assert "L_defer:" in src and "COLD_CALL(cold" not in src
    frame = bytes.fromhex("00112233445566778899aabb0800450000320001000040060000c0a801020a000001123400500000000100000000"
                          "501020000000000080818283848586878889") + bytes(36)
    assert len(frame) == 100 and frame[22] == 64 and frame[56:64].hex() == "8283848586878889"
    buf, off, lens = (skb_packets_to_buffer if skb else packets_to_buffer)([frame])
    run = dict(entry=0, buf=buf, off=off, lens=lens, cpu=np.zeros(1, np.int32), skb=skb)
    out = run_sequence_engine(sc, [run], exec_mode=mode)[0][0]
    want = 0x8283848586878888 if skb else 0x8288878685848382
    got = (int(out["status"][0]), int(out["r0"][0]), int(out["steps"][0]), int(out["err_pc"][0]))
    assert got == (0, want, 9, -1), f"(status, r0, steps, err_pc) = {got[0]}, {got[1]:#x}, {got[2]}, {got[3]}"
    assert out["last_exec"] == mode
    at = int(off[0]) + (32 if skb else 0) + 63
    assert bytes(out["pkt"][at:at + 2]) == (b"\x88\x89" if skb else b"\x82\x83")
