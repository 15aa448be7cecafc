"""ALU, END and jump semantics on MI355X with per-lane operands (tests/opmatrix.py).

The opcode KATs build their operands from immediates and run one packet per batch: both operands are
wave-uniform and the generated code computes on the scalar unit.  Here every program loads its
operands from the packet and runs over 1 024 packets at V = 256, so that the 64 lanes of a wave hold
64 different operand pairs (the edge cross product interleaved with random pairs) and the vector
forms of mul / div / mod / shifts / compares run, lanes that panic (DIV / MOD by a zero register)
beside lanes that go on.

* interpreter and default JIT, one test per (chunk of 40 programs, engine): one batch per program
  with that program as entry, against the oracle running the same sequence (R0, status, steps,
  err_pc, packet memory) and against the model's own arrays;
* Process.Run on the stepping interpreter (MIMIC_PROC_JIT=-1) and on the single-process JIT form
  (MIMIC_PROC_JIT=0): 32 pairs per program, R0 / status / steps / ErrPC against the model.

test_opmatrix_cpu.py holds the oracle to the model and gates the corpus."""
import os

import pytest

import mimic_amd as M
import opmatrix as OM
from harness import assert_same_sequence, build_engine, kernel_of, run_sequence_engine, run_sequence_oracle

pytestmark = pytest.mark.gpu

CHUNKS = OM.chunks()
IDS = [f"chunk{k}_{len(c[1])}" for k, c in enumerate(CHUNKS)]


def jit_kernels():
    """Per chunk the batch kernel and the single-process form (compiled before the session)."""
    out = []
    for _, forms in CHUNKS:
        raws, ctx, vc = kernel_of(OM.scenario(forms))
        out += [(raws, ctx, vc), (raws, ctx | 0x100, vc)]
    return out


_ORACLE = {}


def _oracle(c):
    """The oracle's run of chunk c, computed once for both engines; tests only read it."""
    if c not in _ORACLE:
        _, forms = CHUNKS[c]
        _ORACLE[c] = run_sequence_oracle(OM.scenario(forms), OM.runs(forms))
    return _ORACLE[c]


@pytest.mark.parametrize("mode", ["interp", "jit"])
@pytest.mark.parametrize("c", range(len(CHUNKS)), ids=IDS)
def test_batches(gpu, c, mode):
    first, forms = CHUNKS[c]
    e = run_sequence_engine(OM.scenario(forms), OM.runs(forms), exec_mode=mode)
    for k, out in enumerate(e[0]):
        assert out["last_exec"] == mode, f"{forms[k].name} ran on {out['last_exec']}"
        OM.assert_model(first + k, out, mode)
    assert_same_sequence(_oracle(c), e, tag=f"chunk {c} ({mode})")


def _engine(sc, after):
    old = os.environ.get("MIMIC_PROC_JIT")
    os.environ["MIMIC_PROC_JIT"] = str(after)
    try:
        return build_engine(sc)
    finally:
        if old is None:
            del os.environ["MIMIC_PROC_JIT"]
        else:
            os.environ["MIMIC_PROC_JIT"] = old


@pytest.mark.parametrize("tier", ["interp", "jit"])
@pytest.mark.parametrize("c", range(len(CHUNKS)), ids=IDS)
def test_process_run(gpu, c, tier):
    """One VM per chunk, one process at a time, closed before the next chunk's VM."""
    _, forms = CHUNKS[c]
    vm, _, pids = _engine(OM.scenario(forms), -1 if tier == "interp" else 0)
    try:
        for k, f in enumerate(forms):
            for n, (a, b) in enumerate(OM.PROC_PAIRS):
                p = vm.NewProcess(pids[k], M.LinuxContextXDP(Packet=OM.packet(a, b)))
                p.SetCPUID(n % OM.V_CPUS)
                try:
                    p.Run()
                except M.MimicError:
                    pass
                got = (p.Status, p.Registers.R0, p.Steps, p.ErrPC)
                ran = vm.LastExec()
                p.Cleanup()
                want = OM.model(f, a, b)
                assert got == want, (f"{f.name} ({f.ref}) a={a:#x} b={b:#x} on {ran}: (status, r0, steps, err_pc) "
                                     f"{got} model {want}")
                assert ran == tier, f"{f.name}: Run on {ran}"
    finally:
        vm.close()
