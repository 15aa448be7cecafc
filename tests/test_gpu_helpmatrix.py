"""Map helpers and tail calls on MI355X with per-lane arguments (tests/helpmatrix.py).

Every other helper call of the suite has arguments its generator knows: wave-uniform, so a wave takes
one way through reg_to_map(), load_map()'s readfirstlane branch, readable(), key_fetch(), copy_into(),
the inline lookup / tail-call forms and the translation cache.  Here every program takes one argument
of one call from the packet and runs over 1 024 packets at V = 256, so the 64 lanes of a wave name
different maps, families and key sizes, point keys and values at the inclusive ends of different
entries, index a prog array in range, at E and at 2^32 + 1, and fail with different statuses beside
lanes that go on, continue in another program, or read everything back.

* interpreter and default JIT, one test per (chunk, engine): one VM with four forms' programs and the
  three tail-call targets, one batch per form, against the oracle running the same sequence (R0,
  status, steps, err_pc, packet memory, final map bytes) and against the model's own arrays; the VM
  whose forms insert into and delete from a hash map on many vCPUs at once compares its hash maps by
  key;
* one form per group as a one-program VM (next to the targets), whose kernel calls its cold paths
  inline, and the same with MIMIC_JIT_FAST=0;
* Process.Run on the stepping interpreter (MIMIC_PROC_JIT=-1) and on the single-process JIT form
  (MIMIC_PROC_JIT=0): 32 cases per program, the edge list first, model-exact.

test_helpmatrix_cpu.py holds the oracle to the model and gates the corpus."""
import os

import pytest

import helpmatrix as HM
import mimic_amd as M
from harness import assert_same, build_engine, kernel_of, run_sequence_engine, run_sequence_oracle
from mimic_amd import jit as J

pytestmark = pytest.mark.gpu

CHUNKS = HM.chunks()
FORMS = HM.forms()
IDS = [f"{first:02d}_{fs[0].name}" for first, fs in CHUNKS]
ONE = HM.one_per_group()
ONE_IDS = [FORMS[k].name for k in ONE]


def jit_kernels():
    """Per chunk the batch kernel and the single-process form, and the one-program kernels (compiled
    before the session)."""
    out = []
    for _, fs in CHUNKS:
        raws, ctx, vc = kernel_of(HM.scenario(fs))
        out += [(raws, ctx, vc), (raws, ctx | 0x100, vc)]
    out += [kernel_of(HM.scenario([FORMS[k]])) for k in ONE]
    return out


_ORACLE = {}


def _oracle(key, sc, runs):
    """The oracle's run of a sequence, computed once for every engine; tests only read it."""
    if key not in _ORACLE:
        _ORACLE[key] = run_sequence_oracle(sc, runs)
    return _ORACLE[key]


def _check(fs, want, oracle, e, mode, tag):
    outs, want_maps, want_hashes = want
    for k, out in enumerate(e[0]):
        assert out["last_exec"] == mode, f"{fs[k].name} ran on {out['last_exec']}"
        HM.assert_model(fs, k, outs[k], out, tag)
    HM.assert_model_maps(fs, want_maps, want_hashes, e[1], e[2], tag)
    by_key = any(f.mutates_hash for f in fs)
    for k, (a, b) in enumerate(zip(oracle[0], e[0])):
        try:
            assert_same(dict(a, maps={}, hash={}), dict(b, maps={}, hash={}))
        except AssertionError as ex:
            raise AssertionError(f"{tag} run {k} ({fs[k].name}): {ex}") from None
    assert_same(dict(oracle[0][-1], maps=oracle[1], hash=oracle[2]), dict(e[0][-1], maps=e[1], hash=e[2]), check_pkt=False,
                hash_exact=not by_key)


@pytest.mark.parametrize("mode", ["interp", "jit"])
@pytest.mark.parametrize("c", range(len(CHUNKS)), ids=IDS)
def test_batches(gpu, c, mode):
    first, fs = CHUNKS[c]
    sc, runs = HM.scenario(fs), HM.runs(fs)
    if mode == "jit" and len(fs) == HM.CHUNK:
        src = J.kernel_source(*kernel_of(sc))
        assert "L_defer:" in src and "COLD_CALL(cold" not in src, "the chunk kernels defer their slow paths"
    e = run_sequence_engine(sc, runs, exec_mode=mode)
    _check(fs, HM.expected(c), _oracle(("chunk", c), sc, runs), e, mode, f"{IDS[c]} ({mode})")


_ONE_MODEL = {}


def _one(k, mode_tag):
    fs = [FORMS[k]]
    sc, runs = HM.scenario(fs), HM.runs(fs)
    if k not in _ONE_MODEL:
        _ONE_MODEL[k] = HM.model_sequence(fs)
    e = run_sequence_engine(sc, runs, exec_mode="jit")
    _check(fs, _ONE_MODEL[k], _oracle(("one", k), sc, runs), e, "jit", f"{FORMS[k].name} ({mode_tag})")


@pytest.mark.parametrize("k", ONE, ids=ONE_IDS)
def test_one_program_cold_calls_inline(gpu, k):
    """A one-program set (and the targets): the cold paths are called where they stand, and what
    follows runs in the same kernel with the registers cold_* handed back through the Spill record."""
    src = J.kernel_source(*kernel_of(HM.scenario([FORMS[k]])))
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
        J.prewarm([kernel_of(HM.scenario([FORMS[k]])) for k in ONE])
    finally:
        _env_back("MIMIC_JIT_FAST", old)


@pytest.mark.parametrize("k", ONE, ids=ONE_IDS)
def test_one_program_fast_paths_off(gpu, fast_off_kernels, k, monkeypatch):
    """MIMIC_JIT_FAST=0: every call through the generic helper: a difference that is only there with
    the fast paths on is the inline form's, not helper_*'s."""
    monkeypatch.setenv("MIMIC_JIT_FAST", "0")
    src = J.kernel_source(*kernel_of(HM.scenario([FORMS[k]])))
    assert "lookup_fast" not in src and "tail_fast(" not in src
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
    """One VM per chunk, one process at a time on four vCPUs (rows and hash entries carry over from
    process to process), closed before the next chunk's VM; the model runs the same processes in
    order."""
    first, fs = CHUNKS[c]
    sp = HM.space_of(fs)
    progs = HM.decoded(fs, sp)
    vm, _, pids = _engine(HM.scenario(fs), -1 if tier == "interp" else 0)
    try:
        for k, f in enumerate(fs):
            for n, (pkt, cpu) in enumerate(HM.proc_cases(fs, k)):
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
                want = HM.run_process(sp, progs, k, pkt, 0, 0, cpu)
                d = int.from_bytes(pkt[:8], "little")
                assert got == want[:4], (f"{f.name} ({f.ref}) case {n} delta={d:#x} cpu={cpu} on {ran}: (status, r0, steps, "
                                         f"err_pc) {got} model {want[:4]}")
                assert bytes(mem) == want[4], f"{f.name} case {n} delta={d:#x} on {ran}: packet memory differs"
                assert ran == tier, f"{f.name}: Run on {ran}"
    finally:
        vm.close()
