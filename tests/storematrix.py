"""bpf_skb_store_bytes (helper 9) with per-lane arguments: an address-free model and a corpus.

The oracle answers helper 9 with its engine-helper error, so the engine is held to a model written
against the reference's text, as opmatrix.py, memmatrix.py and helpmatrix.py do for theirs:

* linuxHelperSKBStoreBytes (emulator_linux_helpers.go:608-647), in its order: R1 must resolve to the
  process's *SKBuff (else ctx-access, 26); R3 to a VMMem (else helper-value, 10); make([]byte, R4)
  panics for R4 > 2^48 (slice panic, 27); vmmem.Read(off, value) fails (10) past the entry's backing
  and is "not implemented" for SKBuff / SK / FlowKeys; buf.pkt.Write(uint32(R2), value)
  (memory_plain.go:106-118) fails as a whole (bounds, 5) when uint32(R2) + R4 > 96 + L; R0 = 0.  R5 is
  never read and R1-R5 keep their values (Q8).
* A failing instruction counts as a step and leaves the registers as they were (vm.go:291-340).
* sk_buff packet memory is PlainMemory with ByteOrder BigEndian (emulator_linux_sk_buff.go:108-121):
  LDX / STX through ctx->data and LD_ABS read and write big-endian scalars; Read / Write move bytes.
  Load zeroes the 32-byte headroom and the 64-byte tailroom (context_sk_buff.go:110-119).
* remote_ip4 and sk->src_ip4 are served from what gopacket decoded at Load: a later store into the
  packet does not change them.

The model is address-free.  sk_buff processes leak entries, so every address moves from packet to
packet; here a register holds a number or a pointer (entry, offset), and every pointer a program uses
is formed from R10, ctx, ctx->data, ctx->sk or a lookup result plus a number.  Three layout facts are
used, none an address: the stack entry covers offsets [0, 2048] of a 2048-byte backing with R10 at
256; the sk_buff entry follows it (stack offset 2049 is its first byte); the packet entry covers
[0, 96 + L] of a (96 + L)-byte backing with ctx->data at 32.

Every form's program takes ONE argument of its call from the packet's first 8 bytes (big endian: R2,
the source's offset, R4, or a selector of the source's kind), so the 64 lanes of a wave copy different
lengths to different offsets and fail with different statuses beside lanes that go on.  After the call
it folds R0-R5 (pointers as their distance from where they came from), reads the packet back through
LD_ABS and through ctx->data, and exits with the fold."""
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

import memmatrix as MM  # noqa: E402  (the LDS stack window's size)
import opmatrix as OM  # noqa: E402  (the ALU / jump model)
from mimic_amd import asm as A  # noqa: E402

M64, M32 = (1 << 64) - 1, (1 << 32) - 1
OK, BOUNDS, HELPER_VALUE, CTX_ACCESS, PANIC_SLICE = 0, 5, 10, 26, 27      # include/mimic_amd.h
N_PACKETS, V_CPUS, CHUNK = 1024, 256, 4
FRAME_LENS = (64, 65, 96, 130, 200)
H, T = 32, 64                    # SKBuffFromBytes' headroom and tailroom
STACK_SIZE, FRAME = 2048, 256
SKB_SIZE = 192                   # the sk_buff entry [0, 192]
FAST_MAX = 32                    # runtime.h SKB_STORE_FAST_MAX: the inline form's cap
FOLD_K = MM.FOLD_K
PAT = 0xA1A2A3A4A5A6A7A8         # stack prefill: word k holds PAT + k * PAT_STEP (no two bytes of a run alike)
PAT_STEP = 0x0B0B0B0B
R0_TAG = 0x7E57_0000             # R0 before the call is R0_TAG + the low bits of the lane's argument: never 0
MAP = dict(name="arr", type=2, key_size=4, value_size=16, max_entries=4)
MAP_KEY = 1
MAP_BYTES = MAP["value_size"] * MAP["max_entries"]
SEED = 0x57B9


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Ptr:
    kind: str        # "stack" | "pkt" | "map" | "ctx" | "sk"
    off: int


class State:
    """One sk_buff process: the stack, the packet memory (rooms zeroed at Load) and the array map's
    values (shared by every process of the VM)."""

    def __init__(self, frame: bytes, mapmem: bytearray):
        self.L = len(frame)
        self.load_frame = bytes(frame)                     # what gopacket decoded
        self.stack = bytearray(STACK_SIZE)
        self.pkt = bytearray(H + self.L + T)
        self.pkt[H:H + self.L] = frame
        self.map = mapmem

    def entry(self, p):
        """(backing, offset) of a pointer into a PlainMemory entry, "skb" for one into an entry whose
        Read is not implemented, None for an address no entry holds."""
        if not isinstance(p, Ptr):
            if p & M32 == 0:
                return None                                # the corpus's one unresolved value
            raise ValueError("a number used as an address")
        if p.kind == "stack":
            if 0 <= p.off <= STACK_SIZE:
                return self.stack, p.off
            if STACK_SIZE < p.off <= STACK_SIZE + 1 + SKB_SIZE:
                return "skb"                               # the sk_buff entry follows the stack
        elif p.kind == "pkt" and 0 <= p.off <= len(self.pkt):
            return self.pkt, p.off
        elif p.kind == "map" and 0 <= p.off <= MAP_BYTES:
            return self.map, p.off
        elif p.kind == "ctx" and 0 <= p.off <= SKB_SIZE:
            return "skb"
        elif p.kind == "sk" and 0 <= p.off <= 80:
            return "skb"
        raise ValueError(f"{p}: outside what the model can place")

    def store_bytes(self, r1, r2, r3, r4) -> int:
        """linuxHelperSKBStoreBytes: 0 or the status; the packet memory is written on success only."""
        if not (isinstance(r1, Ptr) and (r1.kind == "ctx" and 0 <= r1.off <= SKB_SIZE or
                                         r1.kind == "stack" and STACK_SIZE < r1.off <= STACK_SIZE + 1 + SKB_SIZE)):
            return CTX_ACCESS                              # :611-619
        e = self.entry(r3)
        if e is None:
            return HELPER_VALUE                            # :623-631
        if r4 > 1 << 48:
            return PANIC_SLICE                             # :633 make([]byte, R4)
        if e == "skb":
            return HELPER_VALUE                            # :634 Read: not implemented
        mem, off = e
        if off + r4 > len(mem):
            return HELPER_VALUE                            # :634 Read past the backing
        value = bytes(mem[off:off + r4])                   # read completely before the write
        at = r2 & M32
        if at + r4 > len(self.pkt):
            return BOUNDS                                  # :639 memory_plain.go:106-118
        self.pkt[at:at + r4] = value
        return OK


def decode(raw: bytes):
    out, i, n = [], 0, len(raw) // 8
    while i < n:
        op, regs = raw[8 * i], raw[8 * i + 1]
        off = int.from_bytes(raw[8 * i + 2:8 * i + 4], "little", signed=True)
        imm = int.from_bytes(raw[8 * i + 4:8 * i + 8], "little", signed=True)
        if op == 0x18:
            v = (imm & M32) | (int.from_bytes(raw[8 * i + 12:8 * i + 16], "little") << 32)
            out += [(op, regs & 15, regs >> 4, off, v), (0, 0, 0, 0, 0)]
            i += 2
            continue
        out.append((op, regs & 15, regs >> 4, off, imm))
        i += 1
    return out


def _ctx_field(st: State, off: int, n: int):
    S = A.SKB
    if n == 4 and off == S["data"]:
        return Ptr("pkt", H)
    if n == 4 and off == S["data_end"]:
        return Ptr("pkt", H + st.L)
    if n == 4 and off == S["len"]:
        return st.L
    if n == 4 and off == S["sk"]:
        return Ptr("sk", 0)
    if n == 4 and off == S["remote_ip4"]:                  # from the Load-time decode; read before and
        return int.from_bytes(st.load_frame[26:30], "little")   # after the call and XORed, so only its
    raise ValueError(f"sk_buff field {off}/{n} is not in the corpus")    # constancy enters R0


def run_process(ins, frame: bytes, mapmem: bytearray):
    """Process.Run of one sk_buff process: (status, R0, steps, err_pc, packet memory)."""
    st = State(frame, mapmem)
    r: List = [0] * 11
    r[1], r[10] = Ptr("ctx", 0), Ptr("stack", FRAME)
    pc = steps = 0
    while True:
        op, dst, src, off, imm = ins[pc]
        steps += 1
        cls = op & 7

        def fail(status):
            assert not isinstance(r[0], Ptr)
            return status, r[0], steps, pc, bytes(st.pkt)

        if op == 0:
            pc += 1
        elif cls == 1 or cls == 2 or cls == 3:             # LDX / ST / STX
            n = (4, 2, 1, 8)[(op >> 3) & 3]
            base = r[src] if cls == 1 else r[dst]
            assert isinstance(base, Ptr), f"pc {pc}: a number as a base"
            p = Ptr(base.kind, base.off + off)
            if p.kind == "ctx":
                assert cls == 1
                r[dst] = _ctx_field(st, p.off, n)
            elif p.kind == "sk":
                assert cls == 1 and n == 4 and p.off == A.SOCK["src_ip4"]
                r[dst] = int.from_bytes(st.load_frame[30:34], "little")
            else:
                mem, o = st.entry(p)
                assert o + n <= len(mem), f"pc {pc}: the corpus's own accesses stay in bounds"
                order = "big" if p.kind == "pkt" else "little"
                if cls == 1:
                    r[dst] = int.from_bytes(mem[o:o + n], order)
                else:
                    v = r[src] if cls == 3 else imm & M64
                    assert not isinstance(v, Ptr)
                    mem[o:o + n] = (v & ((1 << (8 * n)) - 1)).to_bytes(n, order)
            pc += 1
        elif cls == 0 and op != 0x18:                      # LD_ABS (emulator_linux_.go:198-288)
            n = (4, 2, 1, 8)[(op >> 3) & 3]
            assert op & 0xE0 == A.ABS and isinstance(r[6], Ptr) and r[6].kind == "ctx"
            o = H + (imm & M32)
            assert o + n <= len(st.pkt)
            r[0] = int.from_bytes(st.pkt[o:o + n], "big")
            r[1] = r[2] = r[3] = r[4] = r[5] = 0
            pc += 1
        elif op == 0x18:
            r[dst] = imm
            pc += 1
        elif op == 0xBF:
            r[dst] = r[src]
            pc += 1
        elif op == 0xB7:
            r[dst] = imm & M64
            pc += 1
        elif op == 0x95:
            assert not isinstance(r[0], Ptr)
            return OK, r[0], steps, -1, bytes(st.pkt)
        elif op == 0x85:
            if imm == A.FN_MAP_LOOKUP_ELEM:                # the corpus's one lookup: arr[MAP_KEY]
                mem, o = st.entry(r[2])
                k = int.from_bytes(mem[o:o + 4], "little")
                assert k < MAP["max_entries"]
                r[0] = Ptr("map", k * MAP["value_size"])
            else:
                assert imm == A.FN_SKB_STORE_BYTES
                assert not isinstance(r[2], Ptr) and not isinstance(r[4], Ptr)
                status = st.store_bytes(r[1], r[2], r[3], r[4])
                if status:
                    return fail(status)
                r[0] = 0
            pc += 1
        elif isinstance(r[dst], Ptr) or (op & A.X and isinstance(r[src], Ptr)):
            # pointer arithmetic: pointer +- number, the distance of two pointers into one entry
            d, s = r[dst], (r[src] if op & A.X else OM.s32(imm))
            if cls == 5 and op & 0xF8 == A.JEQ and s == 0:         # a lookup result against 0: never null here
                pc += 1
                continue
            assert cls == 7 and op & 0xF0 in (A.ADD, A.SUB), f"pc {pc}: op {op:#x} on a pointer"
            if isinstance(d, Ptr) and isinstance(s, Ptr):
                if d.kind == "stack" and d.off > STACK_SIZE:       # the sk_buff entry follows the stack
                    d = Ptr("ctx", d.off - STACK_SIZE - 1)
                assert op & 0xF0 == A.SUB and d.kind == s.kind
                r[dst] = (d.off - s.off) & M64
            else:
                assert isinstance(d, Ptr)
                r[dst] = Ptr(d.kind, d.off + OM.s64(s) * (1 if op & 0xF0 == A.ADD else -1))
            pc += 1
        else:
            what, v = OM.execute(op, imm, r[dst], r[src] if op & A.X else 0)
            if what == OM.SET:
                r[dst] = v
                pc += 1
            elif what == OM.JUMP:
                pc += 1 + (off if v else 0)
            else:
                raise ValueError(f"opcode {op:#x} is not in the corpus")


# ---------------------------------------------------------------------------------------------
# forms
# ---------------------------------------------------------------------------------------------
def wlo() -> int:
    """Stack offset of the LDS stack window's lower edge (R10 - 128 with the default window)."""
    return FRAME - 8 * MM.lds_q()


def _fold(reg):
    return [A.alu64("mul", 9, FOLD_K), A.alu64("add", 9, reg, reg=True)]


# (stack offset, size) of the src_stack forms' constant-offset stores: written words either side of the
# window's lower edge, of R10 (frame 0 / frame 1), of the fine-granule boundary and at the entry's end,
# a partly written word, and unwritten words between them
def _stack_prefill():
    W = wlo()
    return ((W - 8, 8), (W + 8, 8), (W + 18, 2), (FRAME - 8, 8), (FRAME, 8), (MM.STK_FINE - 8, 8), (MM.STK_FINE + 32, 8),
            (STACK_SIZE - 8, 8))


READBACK_ABS = (0, 20, 36, 60)            # LD_ABS W at these frame offsets
READBACK_DATA = (-32, -8, 0, 16, 32, 56)  # 8 bytes through ctx->data at these offsets (the headroom too)


@dataclass(frozen=True)
class Form:
    name: str
    group: str
    arg: str                  # what the packet's 8 bytes are: "r2" | "r3" | "r4" | "kind"
    n: int = 8                # the constant length (mov immediate); the r4 forms take it from the packet
    src: str = "stack"        # "stack" | "pkt" | "map"
    fixed_r2: int = -1        # twin forms: R2 is this constant, the packet's bytes are unused
    ref: str = "emulator_linux_helpers.go:608-647"

    # source bytes of the r2 / r4 / kind forms: [R10 - 72, R10 - 7], nine prefilled words
    SRC0 = -72

    @functools.cached_property
    def items(self):
        S = A.SKB
        it = [A.mov64_reg(6, 1), A.ldx(4, 7, 6, S["data"]), A.ldx(8, 8, 7, 0), A.ld_imm64(5, PAT)]
        if self.arg == "r3" and self.src == "stack":
            for o, k in _stack_prefill():
                it += [A.stx(k, 10, o - FRAME, 5), A.alu64("add", 5, PAT_STEP)]
        else:
            for q in range(9):
                it += [A.stx(8, 10, self.SRC0 + 8 * q, 5), A.alu64("add", 5, PAT_STEP)]
        it += [A.mov64_reg(9, 8), A.alu64("and", 9, 0xFFFF), A.alu64("add", 9, R0_TAG)]       # R0 before the call
        if self.group == "ipsnap":
            it += [A.ldx(4, 2, 6, S["remote_ip4"]), A.stx(4, 10, -80, 2), A.ldx(4, 3, 6, S["sk"]),
                   A.ldx(4, 2, 3, A.SOCK["src_ip4"]), A.stx(4, 10, -76, 2)]
        if self.group == "barrier":
            it += [A.ld_abs(4, 16), A.jmp("jeq", 0, 0x7FFFFFF1, "out")] + _fold(0)
        if self.src == "map":
            it += [A.st(4, 10, -84, MAP_KEY), A.mov64_reg(2, 10), A.alu64("add", 2, -84), A.ld_map_fd(1, MAP["name"]),
                   A.call(A.FN_MAP_LOOKUP_ELEM), A.jmp("jeq", 0, 0, "out"), A.mov64_reg(3, 0)]
        elif self.src == "pkt":
            it += [A.mov64_reg(3, 7)]
        else:
            it += [A.mov64_reg(3, 10)]
        # the arguments
        it += [A.mov64_reg(1, 6)]
        if self.arg == "r3":
            it += [A.alu64("add", 3, 8, reg=True), A.mov64_imm(2, H + 20)]
        elif self.src == "stack":
            it += [A.alu64("add", 3, self.SRC0)]
        if self.arg == "r2":
            it += [A.mov64_imm(2, self.fixed_r2)] if self.fixed_r2 >= 0 else [A.mov64_reg(2, 8)]
        if self.arg == "r4":
            it += [A.mov64_imm(2, H + 8), A.mov64_reg(4, 8)]
        else:
            it += [A.mov64_imm(4, self.n)]
        it += [A.ld_imm64(5, 0xF1A6_0000_0000_0001)]        # arbitrary flags: never read
        if self.arg == "kind":
            it += [A.mov64_imm(2, H + 12)] + self._kinds()
        it += [A.mov64_reg(0, 9), "call", A.call(A.FN_SKB_STORE_BYTES), "after"]
        # R0 and R1-R5 after the call (Q8): pointers as their distance from their origin
        it += [A.mov64_reg(9, 0), A.alu64("sub", 1, 6, reg=True)] + _fold(1) + _fold(2)
        it += [A.alu64("sub", 3, {"stack": 10, "pkt": 7}.get(self.src, 3), reg=True)] + _fold(3) + _fold(4) + _fold(5)
        if self.group == "two":     # the second call copies what the first wrote, inside the packet, to a higher offset
            it += [A.mov64_reg(1, 6), A.mov64_imm(2, H + 20), A.mov64_reg(3, 7), A.alu64("add", 3, 12), A.mov64_imm(4, 16),
                   A.mov64_imm(5, 0), A.call(A.FN_SKB_STORE_BYTES)] + _fold(0)
        if self.group == "barrier":
            it += [A.jmp("jeq", 9, 0x7FFFFFF2, "out"), A.ld_abs(4, 16)] + _fold(0)
        if self.group == "ipsnap":  # the same fields again: each XORed with what it held before the call
            it += [A.ldx(4, 2, 6, S["remote_ip4"]), A.ldx(4, 3, 10, -80), A.alu64("xor", 2, 3, reg=True)] + _fold(2)
            it += [A.ldx(4, 3, 6, S["sk"]), A.ldx(4, 2, 3, A.SOCK["src_ip4"]), A.ldx(4, 3, 10, -76),
                   A.alu64("xor", 2, 3, reg=True)] + _fold(2)
        for x in READBACK_ABS:
            it += [A.ld_abs(4, x)] + _fold(0)
        for o in READBACK_DATA:
            it += [A.ldx(8, 2, 7, o)] + _fold(2)
        it += [A.mov64_reg(0, 9), A.exit_(), "out", A.mov64_imm(0, 2), A.exit_()]
        return it

    def _kinds(self):
        """r8 selects what R1 / R3 / R4 hold (default: ctx, the stack source, n)."""
        S = A.SKB
        alt = {
            0: [A.mov64_imm(3, 0)],                                          # R3 unresolved
            1: [A.mov64_reg(3, 6)],                                          # R3 = ctx: Read not implemented
            2: [A.ldx(4, 3, 6, S["sk"])],                                    # R3 = ctx->sk: the same
            3: [],                                                           # all good
            4: [A.mov64_reg(1, 10)],                                         # R1 = the stack: no *SKBuff
            5: [A.mov64_imm(1, 0)],                                          # R1 unresolved
            6: [A.alu64("add", 1, 8)],                                       # R1 inside the sk_buff entry: found
            7: [A.mov64_imm(1, 0), A.mov64_imm(3, 0)],                       # both bad: R1 first
            8: [A.mov64_imm(3, 0), A.ld_imm64(4, 1 << 63)],                  # R3 before R4
            9: [A.mov64_reg(3, 6), A.ld_imm64(4, 1 << 63)],                  # R4 before the Read
            10: [A.ld_imm64(4, (1 << 48) + 1)],
            11: [A.ld_imm64(4, 1 << 63)],
            12: [A.mov64_reg(3, 10), A.alu64("add", 3, STACK_SIZE + 1 - FRAME)],     # one past the stack: the sk_buff
            13: [A.mov64_reg(1, 10), A.alu64("add", 1, STACK_SIZE + 1 - FRAME)],     # ... as R1: it IS the *SKBuff
        }
        it = []
        for k, body in alt.items():
            if body:
                it += [A.jmp("jne", 8, k, sum(x.slots for x in body))] + body
        return it

    @functools.cached_property
    def asm(self):
        return A.assemble([x for x in self.items if x not in ("call", "after")])

    @property
    def raw(self):
        return self.asm[0]

    @property
    def relocs(self):
        return self.asm[1]

    def _pc_of(self, label):
        pc = 0
        for x in self.items:
            if x == label:
                return pc
            if not isinstance(x, str):
                pc += x.slots
        raise AssertionError

    @functools.cached_property
    def call_pc(self) -> int:
        return self._pc_of("call")

    @functools.cached_property
    def twin_raw(self) -> bytes:
        """The program with the call replaced by n byte loads through R3 and byte stores through
        ctx->data + R2 - 32, then R0 = 0: what the oracle can run (fixed_r2 forms, in-frame)."""
        assert self.fixed_r2 >= H
        body = []
        for k in range(self.n):
            body += [A.ldx(1, 0, 3, k), A.stx(1, 7, self.fixed_r2 - H + k, 0)]
        body += [A.mov64_imm(0, 0)]
        items = []
        for x in self.items:
            if x == "call":
                items += body
            elif not (isinstance(x, A.Insn) and x.op == (A.JMP | A.CALL) and x.imm == A.FN_SKB_STORE_BYTES):
                items.append(x)
        return A.assemble([x for x in items if x not in ("call", "after")])[0]

    @property
    def twin_extra_steps(self) -> int:
        return 2 * self.n       # 2n + 1 slots for the call's one


CONST_N = (0, 1, 7, 8, 9, FAST_MAX - 1, FAST_MAX, FAST_MAX + 1, 63, 64, 65)


def _forms() -> List[Form]:
    fs = [Form(f"off_n{n}", "off_fast" if 0 < n <= FAST_MAX else "off_cold", "r2", n) for n in CONST_N]
    fs += [Form("len_reg", "len", "r4"),
           Form("src_stack_n8", "src_stack", "r3", 8), Form("src_stack_n24", "src_stack", "r3", 24),
           Form("src_stack_n40", "src_stack", "r3", 40),
           Form("src_pkt_n16", "src_pkt", "r3", 16, "pkt"), Form("src_pkt_n40", "src_pkt", "r3", 40, "pkt"),
           Form("src_map_n8", "src_map", "r3", 8, "map"),
           Form("kind_n4", "kind", "kind", 4),
           Form("two_calls", "two", "r2", 16),
           Form("barrier", "barrier", "r2", 4),
           Form("ipsnap", "ipsnap", "r2", 8)]
    return fs


@functools.lru_cache(maxsize=None)
def forms() -> Tuple[Form, ...]:
    return tuple(_forms())


@functools.lru_cache(maxsize=None)
def chunks():
    """[(first form index, forms)]: CHUNK programs per VM (enough slow-path sites for the kernel to defer)."""
    fs = forms()
    return [(k, list(fs[k:k + CHUNK])) for k in range(0, len(fs), CHUNK)]


def one_per_group() -> List[int]:
    seen, out = set(), []
    for k, f in enumerate(forms()):
        if f.group not in seen:
            seen.add(f.group)
            out.append(k)
    return out


TWINS = (Form("twin_n1", "twin", "r2", 1, fixed_r2=H), Form("twin_n6", "twin", "r2", 6, fixed_r2=H + 6),
         Form("twin_n8", "twin", "r2", 8, fixed_r2=H + 56), Form("twin_n2", "twin", "r2", 2, fixed_r2=H + 24),
         Form("twin_n7", "twin", "r2", 7, fixed_r2=H + 41))


def scenario(fs):
    from harness import Scenario

    init = [("arr", k.to_bytes(4, "little"), map_init(k), 0) for k in range(MAP["max_entries"])]
    return Scenario(vcpus=V_CPUS, maps=[MAP], progs=[(f"p{k}", f.raw, f.relocs) for k, f in enumerate(fs)], map_init=init)


def map_init(k: int) -> bytes:
    return bytes(0x30 + ((k * 37 + 11 * j) % 0x60) for j in range(MAP["value_size"]))


def map_bytes() -> bytearray:
    return bytearray(b"".join(map_init(k) for k in range(MAP["max_entries"])))


# ---------------------------------------------------------------------------------------------
# arguments: the edge list first, then random draws
# ---------------------------------------------------------------------------------------------
def edges(f: Form, L: int) -> List[int]:
    M, n = H + L + T, f.n
    if f.arg == "r2":
        out = [0, H - 1, H, H + L - n, H + L - n + 1, M - n, M - n + 1, M, (1 << 32) + 40, H + 16, H + 26]
        if f.group in ("two", "barrier", "ipsnap"):
            out += [H + 12, H + 14, H + 17, H + 19, H + 24, H + 30]
        return out
    if f.arg == "r4":
        room = STACK_SIZE - (FRAME + f.SRC0)      # what the stack entry holds from the source on: Read fails past it
        return [0, 1, 7, 8, 9, FAST_MAX - 1, FAST_MAX, FAST_MAX + 1, 63, 64, 65, 66, M - (H + 8), M - (H + 8) + 1, 1 << 63,
                (1 << 48) + 1, (1 << 63) + 5, M64, room, room + 1]
    if f.arg == "kind":
        return list(range(14))
    if f.src == "stack":          # offsets from R10
        out = []
        for b in (wlo(), FRAME, MM.STK_FINE):
            out += [b - n, b - n + 1, b - 1, b, b - n // 2]
        out += [wlo() + 16, wlo() + 13, STACK_SIZE - n, STACK_SIZE - n + 1, STACK_SIZE, STACK_SIZE + 1, 0, 3]
        return [o - FRAME for o in out]
    if f.src == "pkt":            # offsets from data; the destination is [H + 20, H + 20 + n)
        return [-H, 20 - n, 20 - n + 1, 20 - 1, 20, 20 + 1, 20 + n - 1, 20 + n, L + T - n, L + T - n + 1, L + T, 0, 20 - n // 2,
                20 + n // 2]
    return [-16, -15, 0, 7, MAP_BYTES - 16 - n, MAP_BYTES - 16 - n + 1, MAP_BYTES - 16]     # from arr[1]


def draw(f: Form, L: int, rng) -> int:
    M, n = H + L + T, f.n
    if f.arg == "r2":
        return rng.randint(0, M + 4)
    if f.arg == "r4":
        return rng.randint(0, M - H)
    if f.arg == "kind":
        return rng.randint(0, 13)
    if f.src == "stack":
        return rng.choice((rng.randint(wlo() - 48, FRAME + 24), rng.randint(MM.STK_FINE - 48, MM.STK_FINE + 48),
                           rng.randint(0, STACK_SIZE + 1))) - FRAME
    if f.src == "pkt":
        return rng.randint(-H, L + T)
    return rng.randint(-16, MAP_BYTES - 16)


def frame(L: int, arg: int, rng) -> bytes:
    """A plain Ethernet / IPv4 / UDP frame of length L whose first 8 bytes (the MAC addresses'
    first) carry the lane's argument, big endian; payload bytes 0x40..0x7f."""
    ip = bytes([0x45, 0]) + (L - 14).to_bytes(2, "big") + b"\x12\x34\x00\x00" + bytes([64, 17, 0, 0]) + \
        bytes(rng.randint(1, 254) for _ in range(8))
    udp = (1000).to_bytes(2, "big") + (2000).to_bytes(2, "big") + (L - 34).to_bytes(2, "big") + b"\0\0"
    f = (arg & M64).to_bytes(8, "big") + bytes(rng.randint(1, 255) for _ in range(4)) + b"\x08\x00" + ip + udp
    return f + bytes(0x40 + rng.randint(0, 0x3F) for _ in range(L - len(f)))


def _batch_of(f: Form, seed: int, n: int, lens=FRAME_LENS):
    rng = random.Random(seed)
    Ls = [lens[k % len(lens)] if k < 2 * len(lens) else rng.choice(lens) for k in range(n)]
    slot = [(H + L + T + 63) // 64 * 64 for L in Ls]
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(slot)[:-1]
    buf = np.random.default_rng(seed).integers(1, 256, int(sum(slot)), dtype=np.uint8)   # dirty rooms: Load zeroes them
    args = []
    for k in range(n):
        e = edges(f, Ls[k])
        a = e[(k // 2) % len(e)] if k % 2 == 0 else draw(f, Ls[k], rng)
        args.append(a & M64)
        o = int(off[k]) + H
        buf[o:o + Ls[k]] = np.frombuffer(frame(Ls[k], a, rng), np.uint8)
    out = dict(skb=True, buf=buf, off=off, lens=np.array(Ls, np.uint32), cpu=(np.arange(n) % V_CPUS).astype(np.int32),
               arg=np.array(args, np.uint64))
    for x in out.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def batch(index: int):
    return _batch_of(forms()[index], SEED * 131 + index, N_PACKETS)


def runs(first: int, fs):
    return [dict(batch(first + k), entry=k) for k in range(len(fs))]


def model_batch(f: Form, b, mapmem: bytearray, raw: bytes = None):
    """The model's run of one batch: status / r0 / steps / err_pc arrays and the final packet buffer."""
    ins = decode(f.raw if raw is None else raw)
    n = len(b["lens"])
    st, r0, steps, epc = np.zeros(n, np.int64), np.zeros(n, np.uint64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    buf = np.array(b["buf"], np.uint8, copy=True)
    for k in range(n):
        o, L = int(b["off"][k]), int(b["lens"][k])
        s = run_process(ins, bytes(buf[o + H:o + H + L]), mapmem)
        st[k], r0[k], steps[k], epc[k] = s[0], s[1], s[2], s[3]
        buf[o:o + H + L + T] = np.frombuffer(s[4], np.uint8)
    d = dict(status=st, r0=r0, steps=steps, err_pc=epc, pkt=buf)
    for x in d.values():
        x.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def expected(index: int):
    """The model's run of form index's batch (computed once; read-only).  No form writes the map."""
    return model_batch(forms()[index], batch(index), map_bytes())


def assert_model(f: Form, b, want, got, tag: str):
    for key in ("status", "r0", "steps", "err_pc"):
        g = np.asarray(got[key]).astype(np.uint64 if key == "r0" else np.int64)
        bad = np.nonzero(g != want[key])[0]
        if len(bad):
            k = int(bad[0])
            raise AssertionError(f"{tag} {f.name} ({f.ref}): {key} differs for {len(bad)} packets, first packet {k} "
                                 f"arg={int(b['arg'][k]):#x} len={int(b['lens'][k])}: got {int(g[k]):#x} model "
                                 f"{int(want[key][k]):#x} (model status {int(want['status'][k])})")
    g = np.asarray(got["pkt"])
    bad = np.nonzero(g[:len(want["pkt"])] != want["pkt"][:len(g)])[0]
    if len(bad):
        k = int(np.searchsorted(b["off"], bad[0], side="right")) - 1
        raise AssertionError(f"{tag} {f.name}: packet memory differs at byte {int(bad[0])} (packet {k} at "
                             f"{int(b['off'][k])}, arg={int(b['arg'][k]):#x}, len={int(b['lens'][k])})")


def proc_cases(index: int, count: int = 32):
    """[(frame, cpu)] of single processes for form index: the edge list first, then random draws."""
    f = forms()[index]
    rng = random.Random(SEED + 7 * index)
    out = []
    for j in range(count):
        L = FRAME_LENS[j % len(FRAME_LENS)]
        e = edges(f, L)
        a = e[j] if j < len(e) else draw(f, L, rng)
        out.append((frame(L, a, rng), j % 4))
    return out
