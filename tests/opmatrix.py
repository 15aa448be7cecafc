"""ALU, END and jump semantics over per-packet operands: a model and a corpus.

The hand KATs (tests/golden/make_golden.py) build every operand with LD_IMM64 / MOV imm and run one
packet per batch, so on the GPU both operands are wave-uniform and the generated code stays on the
scalar unit.  Real programs compute on packet bytes.  Here every program loads its operands from
the packet,

    r2 = *(u32 *)(r1 + 0); r3 = *(u64 *)(r2 + 0); r4 = *(u64 *)(r2 + 8);
    <the instruction on r3, r4 or an immediate>; r0 = r3; exit

(jump programs: `mov r0,0; jcc +1; exit; mov r0,1; exit`, the tail of make_golden.jcase), and runs
over N_PACKETS packets of 16 bytes (a then b, little endian) on V_CPUS vCPUs with cpu[k] = k % V_CPUS.
Under the explicit schedule lane g runs the packets of vCPU g in order (engine.cpp: a stable
counting sort by vCPU; runtime.h pkt_index reads sched_pkts[ex_begin + j]), so in round j the 64
lanes of a wave hold the 64 consecutive packets j * V_CPUS + 64 w .. + 63: 64 different operand
pairs side by side, panicking lanes beside live ones.

The model restates the reference in Python integers and is independent of the oracle and of the
engine (tests/test_opmatrix_cpu.py holds the oracle to it, tests/test_gpu_opmatrix.py the engine):

* ALU (inst_gen.go:7-225): ALU64 `dst OP x`, ALU32 `uint64(uint32(dst) OP uint32(x))`; x is the
  source register or the constant, Constant = int64(int32(imm)), ALU64 takes uint64 of it, ALU32
  uint32.  Go shifts give 0 for counts >= the width (no masking).  DIV / MOD by zero panic (ALU32:
  uint32(x) == 0).
* NEG (inst.go:86-94): ALU32 `uint64(-int32(dst))` sign-extends; both source bits decode to NEG
  (inst.go:25-28: 0x84, 0x8c, 0x87, 0x8f).
* ARSH (inst.go:116-136): `uint64(int32(dst) >> src)` / `uint64(int64(dst) >> src)`: the register
  count is the whole uint64 (not truncated in the 32-bit form), counts >= the width give the sign
  fill, the result sign-extends; a negative constant panics (Go: negative shift amount).
* END (inst.go:138-198, ALU class only, :45-46): 0xd4 assembles LittleEndian from the bytes taken
  most significant first (a byte swap), 0xdc BigEndian from the same bytes (a truncation); imm 64
  reads Uint32 of the first four of eight bytes: the high word (swapped for 0xd4); any other imm
  leaves dst alone.  0xd7 (ALU64 class) has no slot.
* JMP X (inst_gen.go:618-687: the JumpClass register slots hold the instJump32*Reg functions)
  compares the low 32 bits, signed conditions as int32; JSET X is 64-bit (inst.go:53).  JMP K is
  64-bit against uint64(Constant) / Constant.  JMP32 K is 32-bit.  JSET is taken when the AND is
  zero (inst.go:205-241).  Slot 0xff is instJump64JSLEReg (inst_gen.go:686, the last write through
  an invalid opcode).  JMP32 X other than JSET has no slot (unsupported instruction).
"""
from __future__ import annotations

import functools
import os
import random
import sys
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mimic_amd import asm as A  # noqa: E402

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
OK, UNSUP, DIV0, SHIFT = 0, 2, 16, 17      # include/mimic_amd.h

N_PACKETS = 1024
V_CPUS = 256
WAVE = 64
CHUNK = 40


def s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def s64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def bswap(x, nbytes):
    return int.from_bytes((x & ((1 << (8 * nbytes)) - 1)).to_bytes(nbytes, "little"), "big")


# ---------------------------------------------------------------------------------------------
# the model: one instruction of class ALU / ALU64 / JMP / JMP32
# ---------------------------------------------------------------------------------------------
PANIC, SET, JUMP, NOSLOT = "panic", "set", "jump", "noslot"


def _alu(op, imm, d, s):
    is64 = (op & 7) == A.ALU64
    hi = op & 0xF0
    c = s32(imm)                                 # Constant = int64(int32(imm))
    if hi == A.END:
        if is64:
            return NOSLOT, UNSUP                 # inst.go:45-46: only the ALU class slots
        le = not (op & A.X)
        if c == 16:
            return SET, bswap(d, 2) if le else d & 0xFFFF
        if c == 32:
            return SET, bswap(d, 4) if le else d & M32
        if c == 64:
            return SET, bswap(d >> 32, 4) if le else d >> 32
        return SET, d
    if hi == A.NEG:
        return SET, (-d) & M64 if is64 else s32(-s32(d)) & M64
    if hi == A.ARSH:
        if op & A.X:
            n = s                                # the whole uint64
        else:
            if c < 0:
                return PANIC, SHIFT
            n = c
        if is64:
            return SET, (s64(d) >> min(n, 64)) & M64
        return SET, (s32(d) >> min(n, 32)) & M64
    x = s if op & A.X else c & M64
    if is64:
        a, w, m = d, 64, M64
    else:
        a, x, w, m = d & M32, x & M32, 32, M32
    if hi == A.ADD: return SET, (a + x) & m
    if hi == A.SUB: return SET, (a - x) & m
    if hi == A.MUL: return SET, (a * x) & m
    if hi == A.DIV: return (PANIC, DIV0) if x == 0 else (SET, a // x)
    if hi == A.MOD: return (PANIC, DIV0) if x == 0 else (SET, a % x)
    if hi == A.OR: return SET, a | x
    if hi == A.AND: return SET, a & x
    if hi == A.XOR: return SET, a ^ x
    if hi == A.LSH: return SET, 0 if x >= w else (a << x) & m
    if hi == A.RSH: return SET, 0 if x >= w else a >> x
    raise ValueError(f"opcode {op:#x} is not in the corpus")


def _cmp(hi, ua, ub, sa, sb):
    if hi == A.JEQ: return ua == ub
    if hi == A.JGT: return ua > ub
    if hi == A.JGE: return ua >= ub
    if hi == A.JSET: return (ua & ub) == 0       # Q3: taken when no bit is shared
    if hi == A.JNE: return ua != ub
    if hi == A.JSGT: return sa > sb
    if hi == A.JSGE: return sa >= sb
    if hi == A.JLT: return ua < ub
    if hi == A.JLE: return ua <= ub
    if hi == A.JSLT: return sa < sb
    if hi == A.JSLE: return sa <= sb
    raise ValueError(f"jump op {hi:#x}")


def _jmp(op, imm, d, s):
    if op == 0xFF:                               # instJump64JSLEReg
        return JUMP, s64(d) <= s64(s)
    hi = op & 0xF0
    c = s32(imm)
    if (op & 7) == A.JMP:
        if op & A.X:
            if hi == A.JSET:
                return JUMP, (d & s) == 0
            return JUMP, _cmp(hi, d & M32, s & M32, s32(d), s32(s))       # Q1
        return JUMP, _cmp(hi, d, c & M64, s64(d), c)
    if op & A.X:
        if hi == A.JSET:
            return JUMP, (d & s & M32) == 0
        return NOSLOT, UNSUP                     # Q2
    return JUMP, _cmp(hi, d & M32, c & M32, s32(d), s32(c))


def execute(op, imm, d, s):
    """One instruction on dst value d and source-register value s:
    (SET, new dst) | (JUMP, taken) | (PANIC, status) | (NOSLOT, status)."""
    op &= 0xFF
    if op == 0xFF or (op & 7) in (A.JMP, A.JMP32):
        return _jmp(op, imm, d & M64, s & M64)
    return _alu(op, imm, d & M64, s & M64)


# ---------------------------------------------------------------------------------------------
# programs
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Form:
    name: str
    kind: str        # "alu" | "jmp"
    op: int
    imm: int
    ref: str
    cls: str = ""    # jumps: "x" (JMP X), "k" (JMP K), "k32" (JMP32 K), "" otherwise
    cond: str = ""

    @property
    def insn(self):
        return A.raw(self.op, 3, 4, 1 if self.kind == "jmp" else 0, self.imm)

    @property
    def items(self):
        head = [A.ldx(4, 2, 1, 0), A.ldx(8, 3, 2, 0), A.ldx(8, 4, 2, 8)]
        if self.kind == "alu":
            return head + [self.insn, A.mov64_reg(0, 3), A.exit_()]
        return head + [A.mov64_imm(0, 0), self.insn, A.exit_(), A.mov64_imm(0, 1), A.exit_()]

    @property
    def raw(self):
        return A.assemble(self.items)[0]


def model(f: Form, a: int, b: int) -> Tuple[int, int, int, int]:
    """(status, r0, steps, err_pc) of form f's program on the packet (a, b).  steps counts the
    calls of Process.Step (vm.go:291), the failing one included (make_golden.py div64_x_zero: 3 steps,
    err_pc 2); a failing instruction leaves R0 as it was: 0."""
    what, v = execute(f.op, f.imm, a, b)
    at = 3 if f.kind == "alu" else 4
    if what in (PANIC, NOSLOT):
        return v, 0, at + 1, at
    if what == SET:
        return OK, v, 6, -1
    return OK, int(v), 7 if v else 6, -1


ALU_X_OPS = ("add", "sub", "mul", "div", "mod", "or", "and", "xor", "lsh", "rsh", "arsh", "neg")
SHIFT_IMMS = (0, 1, 31, 32, 33, 63, 64, -1)
DIV_IMMS = (0, 1, -1, 3, 0x7FFFFFFF, -0x80000000)
REST_IMMS = (-1, -0x80000000, 0x7FFFFFFF, 0x12345678)
JMP_IMMS = (0, -1, 0x7FFFFFFF, -0x80000000)
CONDS = ("jeq", "jgt", "jge", "jset", "jne", "jsgt", "jsge", "jlt", "jle", "jslt", "jsle")


def _imm_name(i):
    return f"{i & M32:x}"


def _forms() -> List[Form]:
    out = []
    for w, cls in (("alu64", A.ALU64), ("alu32", A.ALU)):
        for op in ALU_X_OPS:    # NEG with the register bit set is NEG all the same (0x8f, 0x8c)
            ref = "inst.go:116-136" if op == "arsh" else "inst.go:25-28,86-94" if op == "neg" else "inst_gen.go:7-225"
            out.append(Form(f"{w}_{op}_x", "alu", cls | A.ALU_OPS[op] | A.X, 0, ref))
    out.append(Form("alu64_neg", "alu", A.ALU64 | A.NEG, 0, "inst.go:91-94"))
    out.append(Form("alu32_neg", "alu", A.ALU | A.NEG, 0, "inst.go:86-89"))
    out.append(Form("alu64_neg_imm_ignored", "alu", A.ALU64 | A.NEG, 7, "inst.go:91-94"))
    for w, cls in (("alu64", A.ALU64), ("alu32", A.ALU)):
        for op in ("lsh", "rsh", "arsh"):
            for i in SHIFT_IMMS:
                out.append(Form(f"{w}_{op}_k_{_imm_name(i)}", "alu", cls | A.ALU_OPS[op], i,
                                "inst.go:116-130" if op == "arsh" else "inst_gen.go:139-169"))
        for op in ("div", "mod"):
            for i in DIV_IMMS:
                out.append(Form(f"{w}_{op}_k_{_imm_name(i)}", "alu", cls | A.ALU_OPS[op], i, "inst_gen.go:73-81,183-191"))
        for op in ("add", "sub", "mul", "or", "and", "xor"):
            for i in REST_IMMS:
                out.append(Form(f"{w}_{op}_k_{_imm_name(i)}", "alu", cls | A.ALU_OPS[op], i, "inst_gen.go:7-225"))
    for i in (16, 32, 64, 8):
        out.append(Form(f"end_le_{i}", "alu", 0xD4, i, "inst.go:138-167"))
        out.append(Form(f"end_be_{i}", "alu", 0xDC, i, "inst.go:169-198"))
    out.append(Form("end_alu64_class", "alu", 0xD7, 16, "inst.go:45-46"))
    for c in CONDS:
        out.append(Form(f"{c}_x", "jmp", A.JMP | A.JMP_OPS[c] | A.X, 0,
                        "inst.go:53,233-241" if c == "jset" else "inst_gen.go:618-687 (Q1)", "x", c))
    out.append(Form("slot_0xff_x", "jmp", 0xFF, 0, "inst_gen.go:686", "x", "jsle64"))
    out.append(Form("jset32_x", "jmp", A.JMP32 | A.JSET | A.X, 0, "inst.go:51,223-231", "x", "jset32"))
    out.append(Form("jsgt32_x_no_slot", "jmp", A.JMP32 | A.JSGT | A.X, 0, "inst_gen.go:654 keys JumpClass (Q2)"))
    for cname, cls in (("k", A.JMP), ("k32", A.JMP32)):
        for c in CONDS:
            for i in JMP_IMMS:
                out.append(Form(f"{c}_{cname}_{_imm_name(i)}", "jmp", cls | A.JMP_OPS[c], i,
                                "inst.go:205-221" if c == "jset" else "inst_gen.go:227-605", cname, c))
    names = [f.name for f in out]
    assert len(set(names)) == len(names)
    return out


FORMS = _forms()
DIV_X = [f for f in FORMS if f.kind == "alu" and f.op & A.X and (f.op & 0xF0) in (A.DIV, A.MOD)]


def chunks():
    """[(first form index, forms)]: CHUNK programs to a VM, as kat.jit_groups does."""
    return [(a, FORMS[a:a + CHUNK]) for a in range(0, len(FORMS), CHUNK)]


# ---------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------
EDGES = [0, 1, 5, 31, 32, 33, 63, 64, 65,
         0x7FFFFFFF, 0x80000000, 0xFFFFFFFF,
         0x1_0000_0000, 0x1_0000_0001, 0x1_0000_0020,
         (1 << 63) - 1, 1 << 63, M64,
         0x123456789ABCDEF0, 0xFFFFFFFF00000000, 0xFFFFFFFF80000000, 0x11223344AABBCCDD]
SEED = 0x0B1A5


@functools.lru_cache(maxsize=None)
def pairs() -> Tuple[Tuple[int, int], ...]:
    """The N_PACKETS operand pairs.  Even packets walk EDGES x EDGES with b as the fast index (any
    32 consecutive slots cycle through every b); odd packets are seeded random pairs whose bit
    lengths are uniform in 1..64, so quotients of every size occur."""
    rng = random.Random(SEED)
    E = len(EDGES)
    assert N_PACKETS // 2 >= E * E
    out = []
    for k in range(N_PACKETS):
        if k % 2 == 0:
            e = k // 2
            out.append((EDGES[(e // E) % E], EDGES[e % E]))
        else:
            out.append((_bits(rng), _bits(rng)))
    return tuple(out)


def _bits(rng):
    """A random value of a bit length drawn uniformly from 1..64."""
    n = rng.randint(1, 64)
    return (1 << (n - 1)) | rng.getrandbits(n - 1) if n > 1 else 1


# Process.Run: the edge diagonal and ten pairs whose b makes DIV / MOD panic (b == 0, and b != 0
# with uint32(b) == 0), their a's of both signs in both widths
PROC_PAIRS = tuple([(v, v) for v in EDGES] +
                   [(5, 0), (1 << 63, 0), (M64, 0), (0x80000000, 0), (0x123456789ABCDEF0, 0),
                    (7, 0x1_0000_0000), (0xFFFFFFFF80000000, 0x1_0000_0000), (0x7FFFFFFF, 0xFFFFFFFF00000000),
                    (0x11223344AABBCCDD, 0xFFFFFFFF00000000), ((1 << 63) - 1, 0x1_0000_0000)])
assert len(PROC_PAIRS) == 32


def packet(a: int, b: int) -> bytes:
    return (a & M64).to_bytes(8, "little") + (b & M64).to_bytes(8, "little")


@functools.lru_cache(maxsize=None)
def batch():
    """The one batch every program runs: (buf, off, lens, cpu), each packet in a 64-byte cell.  The
    runners copy it (the oracle a host copy, the engine to the device); nobody writes it."""
    stride = 64
    buf = np.zeros(N_PACKETS * stride, np.uint8)
    for k, (a, b) in enumerate(pairs()):
        buf[k * stride:k * stride + 16] = np.frombuffer(packet(a, b), np.uint8)
    off = (np.arange(N_PACKETS) * stride).astype(np.uint64)
    lens = np.full(N_PACKETS, 16, np.uint32)
    cpu = (np.arange(N_PACKETS) % V_CPUS).astype(np.int32)
    return buf, off, lens, cpu


@functools.lru_cache(maxsize=None)
def expected(index: int):
    """The model's verdicts for FORMS[index] over pairs(): dict of read-only arrays."""
    f = FORMS[index]
    rows = [model(f, a, b) for a, b in pairs()]
    out = dict(status=np.array([r[0] for r in rows], np.int64), r0=np.array([r[1] for r in rows], np.uint64),
               steps=np.array([r[2] for r in rows], np.int64), err_pc=np.array([r[3] for r in rows], np.int64))
    for x in out.values():
        x.setflags(write=False)
    return out


def scenario(forms):
    from harness import Scenario

    return Scenario(vcpus=V_CPUS, maps=[], progs=[(f"p{k}", f.raw, []) for k, f in enumerate(forms)])


def runs(forms):
    buf, off, lens, cpu = batch()
    return [dict(entry=k, buf=buf, off=off, lens=lens, cpu=cpu) for k in range(len(forms))]


def assert_model(index: int, got, tag: str):
    """got: a result dict (r0 / status / steps / err_pc arrays) against expected(index)."""
    want = expected(index)
    for key in ("status", "r0", "steps", "err_pc"):
        g = np.asarray(got[key]).astype(np.uint64 if key == "r0" else np.int64)
        bad = np.nonzero(g != want[key])[0]
        if len(bad):
            k = int(bad[0])
            a, b = pairs()[k]
            raise AssertionError(f"{tag} {FORMS[index].name} ({FORMS[index].ref}): {key} differs for {len(bad)} packets, "
                                 f"first packet {k} a={a:#x} b={b:#x}: got {int(g[k]):#x} model {int(want[key][k]):#x}")
