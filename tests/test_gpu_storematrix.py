"""bpf_skb_store_bytes on MI355X with per-lane arguments (tests/storematrix.py).

Every program takes one argument of its call from the packet and runs over 1 024 packets at V = 256
with frame lengths mixed from {64, 65, 96, 130, 200}: the 64 lanes of a wave copy different lengths
from different sources to different offsets, into both rooms and across the frame's ends, and fail
with different statuses beside lanes that go on.  Everything is compared with the model: R0, status,
steps, err_pc and every byte of packet memory, rooms included.

* interpreter and default JIT, one test per (chunk, engine): one VM with the chunk's programs, one
  batch per form; the chunk kernels defer their slow paths (the resume kernel runs the helper);
* one form per group as a one-program VM, whose kernel calls cold_store_bytes inline, and the same with
  MIMIC_JIT_FAST=0 and with MIMIC_JIT_SKBSTORE=0 (a difference that is only there with a knob on is the
  inline form's);
* Process.Run under MIMIC_PROC_JIT=-1 and =0 (sk_buff processes run on the stepping interpreter under
  both), one Process.Step trace through a call, one pooled run (mimic_process_run_many);
* two batches over one SKBBatch buffer: the first writes room bytes through the helper, the second
  must find the rooms zeroed again;
* an xdp_md VM calling helper 9: ctx-access on every engine;
* workloads.prog_skb_rewrite against prog_skb_rewrite_direct, the oracle and the numpy expectation.

test_storematrix_cpu.py holds the model to hand-worked cases and to the oracle."""
import os
import threading
import time

import numpy as np
import pytest

import mimic_amd as M
import storematrix as SM
from harness import Scenario, build_engine, kernel_of, run_engine, run_engine_skb, run_oracle_skb, run_sequence_engine
from mimic_amd import asm as A
from mimic_amd import jit as J
from mimic_amd import workloads as W

pytestmark = pytest.mark.gpu

CHUNKS = SM.chunks()
FORMS = SM.forms()
IDS = [f"{first:02d}_{fs[0].name}" for first, fs in CHUNKS]
ONE = SM.one_per_group()
ONE_IDS = [FORMS[k].name for k in ONE]
REWRITE_N = 16384


def _xdp_raw():
    """An xdp_md program calling helper 9 with arguments that would be fine on an sk_buff."""
    return A.assemble([A.mov64_imm(0, 77), A.stx(8, 10, -8, 0), A.mov64_imm(2, 0), A.mov64_reg(3, 10), A.alu64("add", 3, -8),
                       A.mov64_imm(4, 4), A.mov64_imm(5, 0), A.call(A.FN_SKB_STORE_BYTES), A.exit_()])[0]


def jit_kernels():
    out = [kernel_of(SM.scenario(fs), J.CTX_SKB) for _, fs in CHUNKS]
    out += [kernel_of(SM.scenario([FORMS[k]]), J.CTX_SKB) for k in ONE]
    out += [([W.prog_skb_rewrite().raw], J.CTX_SKB, []), ([W.prog_skb_rewrite_direct().raw], J.CTX_SKB, []),
            ([_xdp_raw()], J.CTX_XDP, []), ([_xdp_raw()], J.CTX_XDP | 0x100, [])]
    return out


def _check(fs, first, e, mode, tag):
    for k, out in enumerate(e[0]):
        assert out["last_exec"] == mode, f"{fs[k].name} ran on {out['last_exec']}"
        SM.assert_model(fs[k], SM.batch(first + k), SM.expected(first + k), out, tag)
    assert [bytes(v) for v in e[1]["arr"]] == [bytes(SM.map_bytes())], "no form writes the map"


@pytest.mark.parametrize("mode", ["interp", "jit"])
@pytest.mark.parametrize("c", range(len(CHUNKS)), ids=IDS)
def test_batches(gpu, c, mode):
    first, fs = CHUNKS[c]
    sc = SM.scenario(fs)
    if mode == "jit":
        src = J.kernel_source(*kernel_of(sc, J.CTX_SKB))
        assert "L_defer:" in src and "COLD_CALL(cold" not in src, "the chunk kernels defer their slow paths"
    e = run_sequence_engine(sc, SM.runs(first, fs), exec_mode=mode)
    _check(fs, first, e, mode, f"{IDS[c]} ({mode})")


def _one(k, tag):
    fs = [FORMS[k]]
    e = run_sequence_engine(SM.scenario(fs), SM.runs(k, fs), exec_mode="jit")
    _check(fs, k, e, "jit", f"{FORMS[k].name} ({tag})")


@pytest.mark.parametrize("k", ONE, ids=ONE_IDS)
def test_one_program_cold_calls_inline(gpu, k):
    src = J.kernel_source(*kernel_of(SM.scenario([FORMS[k]]), J.CTX_SKB))
    assert "COLD_CALL(cold_store_bytes" in src and "L_defer:" not in src and "#define MIMIC_COLD_INLINE 1" in src
    # (the kind form's branches lie between its `mov r4, n` and the call: another basic block)
    assert ("store_bytes_fast" in src) == (FORMS[k].arg not in ("r4", "kind") and 0 < FORMS[k].n <= SM.FAST_MAX)
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


def _knob_kernels(name):
    """The knob is read when a kernel is generated, which the session prewarm did without it."""
    old = _env(name, "0")
    try:
        J.prewarm([kernel_of(SM.scenario([FORMS[k]]), J.CTX_SKB) for k in ONE])
    finally:
        _env_back(name, old)


@pytest.fixture(scope="module")
def fast_off_kernels(gpu):
    _knob_kernels("MIMIC_JIT_FAST")


@pytest.fixture(scope="module")
def skbstore_off_kernels(gpu):
    _knob_kernels("MIMIC_JIT_SKBSTORE")


@pytest.mark.parametrize("k", ONE, ids=ONE_IDS)
def test_one_program_fast_paths_off(gpu, fast_off_kernels, k, monkeypatch):
    monkeypatch.setenv("MIMIC_JIT_FAST", "0")
    assert "store_bytes_fast" not in J.kernel_source(*kernel_of(SM.scenario([FORMS[k]]), J.CTX_SKB))
    _one(k, "MIMIC_JIT_FAST=0")


@pytest.mark.parametrize("k", ONE, ids=ONE_IDS)
def test_one_program_inline_form_off(gpu, skbstore_off_kernels, k, monkeypatch):
    monkeypatch.setenv("MIMIC_JIT_SKBSTORE", "0")
    assert "store_bytes_fast" not in J.kernel_source(*kernel_of(SM.scenario([FORMS[k]]), J.CTX_SKB))
    _one(k, "MIMIC_JIT_SKBSTORE=0")


def _engine(sc, after):
    old = _env("MIMIC_PROC_JIT", str(after))
    try:
        return build_engine(sc, ctx=1)
    finally:
        _env_back("MIMIC_PROC_JIT", old)


@pytest.mark.parametrize("after", [-1, 0], ids=["proc_jit_off", "proc_jit_at_once"])
@pytest.mark.parametrize("c", range(len(CHUNKS)), ids=IDS)
def test_process_run(gpu, c, after):
    """One VM per chunk, one process at a time, 32 cases per form (the edge list first); sk_buff
    processes run on the stepping interpreter whatever MIMIC_PROC_JIT says."""
    first, fs = CHUNKS[c]
    vm, _, pids = _engine(SM.scenario(fs), after)
    try:
        for k, f in enumerate(fs):
            ins = SM.decode(f.raw)
            for n, (frame, cpu) in enumerate(SM.proc_cases(first + k)):
                p = vm.NewProcess(pids[k], M.LinuxContextSKBuff(Packet=frame))
                p.SetCPUID(cpu)
                try:
                    p.Run()
                except M.MimicError:
                    pass
                got = (p.Status, p.Registers.R0, p.Steps, p.ErrPC)
                mem = p.Packet()
                ran = vm.LastExec()
                p.Cleanup()
                want = SM.run_process(ins, frame, SM.map_bytes())
                arg = int.from_bytes(frame[:8], "big")
                assert got == want[:4], (f"{f.name} case {n} arg={arg:#x} len={len(frame)} on {ran}: (status, r0, steps, err_pc) "
                                         f"{got} model {want[:4]}")
                assert bytes(mem) == want[4], f"{f.name} case {n} arg={arg:#x}: packet memory differs"
                assert ran == "interp", f"{f.name}: Run on {ran}"
    finally:
        vm.close()


def test_process_step_through_a_call(gpu):
    """Process.Step over off_n8 (straight-line: step s runs slot s - 1): packet memory is the loaded
    packet until the call's step and the model's final packet from it on; R0 is 0 right after it."""
    import random

    f = FORMS[[x.name for x in FORMS].index("off_n8")]
    frame = SM.frame(96, 28, random.Random(3))                 # [28, 36): the headroom's end and the frame's start
    want = SM.run_process(SM.decode(f.raw), frame, SM.map_bytes())
    loaded = bytes(32) + frame + bytes(64)
    assert want[0] == 0 and want[4] != loaded
    vm, _, pids = build_engine(SM.scenario([f]), ctx=1)
    try:
        p = vm.NewProcess(pids[0], M.LinuxContextSKBuff(Packet=frame))
        p.SetCPUID(1)
        s, done = 0, False
        while not done:
            done = p.Step()
            s += 1
            assert p.Packet() == (loaded if s <= f.call_pc else want[4]), f"after step {s}"
            if s == f.call_pc + 1:
                assert p.Registers.R0 == 0 and p.Registers.R2 == 28 and p.Registers.R4 == 8
        assert (p.Status, p.Registers.R0, p.Steps) == (0, want[1], want[2]) and s == want[2]
        p.Cleanup()
    finally:
        vm.close()


def test_pooled_processes(gpu):
    """64 jobs through the process pool (micro-batched launches of NewProcess'd processes,
    mimic_process_run_many) on a VM whose batch interpreter instance carries the helper."""
    k = [x.name for x in FORMS].index("off_n9")
    f = FORMS[k]
    cases = SM.proc_cases(k, 64)
    vm, _, pids = build_engine(Scenario(vcpus=16, maps=[SM.MAP], progs=[("p0", f.raw, f.relocs)]), ctx=1)
    try:
        procs = [vm.NewProcess(pids[0], M.LinuxContextSKBuff(Packet=fr)) for fr, _ in cases]
        pool = vm.GetProcessPool()
        pool.Start(len(procs))
        got, mu = {}, threading.Lock()

        def handoff(proc, err):
            with mu:
                got[proc.idx] = (proc.Status, proc.Registers.R0, proc.Steps, proc.Packet())
            proc.Cleanup()

        for i, p in enumerate(procs):
            p.idx = i
            pool.Enqueue(M.ProcessPoolJob(p, None, handoff))
        pool.Stop()
        t0 = time.time()
        while len(got) < len(procs) and time.time() - t0 < 60:
            time.sleep(0.01)
        assert len(got) == len(procs)
        ins = SM.decode(f.raw)
        for i, (fr, _) in enumerate(cases):
            want = SM.run_process(ins, fr, SM.map_bytes())
            assert got[i][:3] == want[:3], (i, got[i][:3], want[:3])
            assert got[i][3] == want[4], i
    finally:
        vm.close()


@pytest.mark.parametrize("mode", ["interp", "jit"])
def test_two_batches_over_one_buffer(gpu, mode):
    """The first batch writes head- and tailroom bytes through the helper (the interpreter's, or the
    one-program kernel's cold_store_bytes: the inline form takes frame-only stores), which marks the
    batch's rooms-clean word, so the second batch over the same device buffer finds the rooms zeroed
    again (context_sk_buff.go:110-119) -- its read-back of the headroom and its final packet memory
    say so."""
    k = [x.name for x in FORMS].index("off_n8")
    f, b = FORMS[k], SM.batch(k)
    first = SM.expected(k)
    second_in = dict(b, buf=first["pkt"])
    second = SM.model_batch(f, second_in, SM.map_bytes())
    assert not np.array_equal(second["r0"], first["r0"]) and not np.array_equal(second["pkt"], first["pkt"])
    vm, _, pids = build_engine(SM.scenario([f]), ctx=1, exec_mode=mode)
    try:
        sb = M.SKBBatch.from_numpy(b["buf"], b["off"], b["lens"], "cuda:0", 0, M.SCHED_EXPLICIT, b["cpu"], 0, None)
        for want, src, tag in ((first, b, "first"), (second, second_in, "second")):
            o = vm.RunSKBBatch(pids[0], sb).numpy(len(b["lens"]))
            o["pkt"] = sb.pkt_data.cpu().numpy()
            assert vm.LastExec() == mode
            SM.assert_model(f, src, want, o, f"{tag} batch ({mode})")
    finally:
        vm.close()


def test_xdp_vm_answers_ctx_access(gpu):
    """An xdp_md VM has no *SKBuff: status 26 at the call on the interpreter, the JIT and Process.Run,
    R0 and the packet untouched."""
    raw = _xdp_raw()
    sc = Scenario(vcpus=8, progs=[("x9", raw, [])])
    buf, off, lens = W.make_packets(256)
    cpu = (np.arange(256) % 8).astype(np.int32)
    for mode in ("interp", "jit"):
        e = run_engine(sc, buf, off, lens, cpu, exec_mode=mode)
        assert e["last_exec"] == mode
        assert (e["status"] == SM.CTX_ACCESS).all() and (e["r0"] == 77).all() and (e["err_pc"] == 7).all() and (e["steps"] == 8).all()
        assert np.array_equal(e["pkt"][:len(buf)], buf)
    # Process.Run on the stepping interpreter, and on the single-process JIT form (MIMIC_PROC_JIT=0: an
    # xdp_md process is the one that tiers up), whose kernel meets the call through cold_store_bytes
    for after, tier in ((-1, "interp"), (0, "jit")):
        old = _env("MIMIC_PROC_JIT", str(after))
        try:
            vm, _, pids = build_engine(sc)
        finally:
            _env_back("MIMIC_PROC_JIT", old)
        try:
            for n in range(3):
                p = vm.NewProcess(pids[0], M.LinuxContextXDP(Packet=bytes(range(64))))
                p.SetCPUID(n)
                with pytest.raises(M.MimicError):
                    p.Run()
                assert (p.Status, p.Registers.R0, p.Steps, p.ErrPC) == (SM.CTX_ACCESS, 77, 8, 7), (tier, n)
                assert p.Packet() == bytes(range(64)) and vm.LastExec() == tier, (tier, vm.LastExec())
                p.Cleanup()
        finally:
            vm.close()


_REWRITE = {}


def _rewrite_reference():
    """The batch, the oracle's run of the direct program and the numpy expectation (computed once)."""
    if not _REWRITE:
        buf, off, lens = W.make_skb_packets(REWRITE_N, sizes=SM.FRAME_LENS, weights=(1,) * 5, variety=0.3)
        cpu = (np.arange(REWRITE_N) % SM.V_CPUS).astype(np.int32)
        d = W.prog_skb_rewrite_direct()
        o = run_oracle_skb(Scenario(vcpus=SM.V_CPUS, progs=[(d.name, d.raw, d.relocs)]), buf, off, lens, cpu)
        exp, r0 = W.skb_rewrite_expected(buf, off, lens)
        ok = np.asarray(o["status"]) == 0
        assert np.array_equal(np.asarray(o["r0"]).astype(np.uint64)[ok], r0[ok]) and (r0[ok] > 0).sum() > REWRITE_N // 2
        for i in np.nonzero(~ok)[0]:                       # a failed Load leaves its packet memory as it was
            a, b = int(off[i]), int(off[i]) + 96 + int(lens[i])
            exp[a:b] = buf[a:b]
        assert np.array_equal(o["pkt"][:len(exp)], exp[:len(o["pkt"])]), "the oracle's packets against the numpy expectation"
        _REWRITE.update(buf=buf, off=off, lens=lens, cpu=cpu, oracle=o)
    return _REWRITE


@pytest.mark.parametrize("mode", ["interp", "jit"])
def test_rewrite_workloads(gpu, mode):
    """prog_skb_rewrite (helper 9) and prog_skb_rewrite_direct (byte stores through ctx->data) leave
    identical packet memory, R0 and status, equal to the oracle's run of the direct program (which
    workloads.skb_rewrite_expected was checked against)."""
    R = _rewrite_reference()
    o = R["oracle"]
    outs = {}
    for p in (W.prog_skb_rewrite(), W.prog_skb_rewrite_direct()):
        sc = Scenario(vcpus=SM.V_CPUS, progs=[(p.name, p.raw, p.relocs)])
        e = run_engine_skb(sc, R["buf"], R["off"], R["lens"], R["cpu"], exec_mode=mode)
        assert e["last_exec"] == mode, p.name
        assert np.array_equal(e["status"], o["status"]), p.name
        assert np.array_equal(np.asarray(e["r0"]).astype(np.uint64), np.asarray(o["r0"]).astype(np.uint64)), p.name
        assert np.array_equal(e["pkt"][:len(o["pkt"])], o["pkt"][:len(e["pkt"])]), f"{p.name}: packet memory differs from the oracle's"
        outs[p.name] = e
    a, b = outs["skb_rewrite"], outs["skb_rewrite_direct"]
    assert np.array_equal(a["pkt"], b["pkt"]) and np.array_equal(a["r0"], b["r0"])
    assert np.array_equal(np.asarray(b["steps"]), np.asarray(o["steps"])) and np.array_equal(np.asarray(b["err_pc"]), np.asarray(o["err_pc"]))
