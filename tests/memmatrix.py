"""Load and store semantics over per-packet addresses: a model of the address space and a corpus.

Every memory access of the other modules has an address its generator knows when it builds the
program: the memory KATs (tests/golden/make_golden.py layout_*, xdp_md_*, stack_*, packet_*) run one
packet per batch at constant offsets, test_gpu_fastpaths.test_lds_stack_window walks a fixed list of
R10 + k, test_gpu_vc.py compiles one program per (offset, size), fuzz_struct.py loads the packet at
constant offsets behind a bounds check.  Here every program takes its address from the packet:

    r6 = r1; r2 = data; r3 = data_end; if (r2 + 16 > r3) goto out
    [map regions: *(u32 *)(r10 - 4) = key; r0 = lookup(map, r10 - 4); if (!r0) goto out; r1 = r0]
    r7 = (s64)*(s32 *)(r2 + 0) + ((u64)*(u32 *)(r2 + 4) << 32)      the delta, bits 32..63 apart
    r8 = *(u64 *)(r2 + 8) ^ VALUE_FLIP; r5 = PREFILL; r0 = r8
    a few stores at constant offsets (through r10: they switch the LDS stack window on and leave
    partly valid words either side of its lower edge; through the lookup result: the row)
    r9 = base; r9 += r7
    the access: r4 = *(uN *)(r9 + 0)  |  *(uN *)(r9 + 0) = r8  |  *(uN *)(r9 + 0) = IMM
    (rows: the row as the vCPU's previous packet left it is folded into r0 before those stores)
    stores: r4 = *(uN *)(r9 + 0) again (the bytes back through the same address); r0 = r0 * K + r4
    read back at constant offsets, each folded as r0 = r0 * K + r4: R10 words around every stack
    boundary, the xdp_md fields through r6, data / data_end reloaded, the packet's first 16 bytes,
    the row's words
    exit                                                              (out: r0 = 2; exit)

and runs over N_PACKETS packets on V_CPUS vCPUs with cpu[k] = k % V_CPUS, so that the 64 lanes of a
wave hold 64 consecutive packets (tests/opmatrix.py has the argument): 64 different addresses side by
side, landing in different entries and leaving through different error exits.  R0 is never zero when
a packet fails in the access (the value, folded with the row in the row forms), so an error exit that
loses R0 shows.

The model restates the reference in Python integers and bytearrays.  It is independent of the oracle
and of the engine (tests/test_memmatrix_cpu.py holds the oracle to it, tests/test_gpu_memmatrix.py
the engine):

* MemoryController.AddEntry (memory_controller.go:58-112): first fit from 0x10000; an entry of size
  s at A covers [A, A + s] INCLUSIVE and the next one starts at A + s + 1 (the layout_* KATs pin
  this).  Static entries in API order: array = object (8) + values (E * S);
  per-CPU array = object (8) + V x [sub-array object (8), values]; hash = object (8), keys (E * K),
  values (E * S); program = object (8).
* Per process (vm.go:198-235, context_xdp_md.go:47-115): stack [St, St + 2048] with R10 = St + 256,
  packet [P, P + M] with M = H + L + T and the rooms zeroed, xdp_md [X, X + 24] holding data = P + H,
  data_end = P + H + L, data_meta = P + H and the three indexes; Cleanup frees them, so every
  process gets the same addresses (the packet's length moves X).
* GetEntry (memory_controller.go:117-145): the entry with Addr <= a <= Addr + Size.
* LDX / STX / ST (inst.go:298-363): addr := uint32(reg + off); no entry: unresolved; an entry whose
  object is no VMMem (a hash or per-CPU array object, a program): not-VMMem; an array object whose
  spec is no datasec (emulator_linux_map_array.go:136-138): not-datasec; PlainMemory.Load / Store
  (memory_plain.go:25-87): off + n > len(backing) is out of bounds -- so the byte A + s resolves and
  then fails for every size -- little endian otherwise.  ST stores uint64(Constant) with
  Constant = int64(int32(imm)): the sign extension fills an 8-byte store.
* A failing instruction counts as a step and leaves the registers as they were (vm.go:291-340).
* bpf_map_lookup_elem (emulator_linux_helpers.go:477-504): R1 names the map's object, the key is
  read from R2; array: key >= E gives 0, else values + key * S (per-CPU: of the process's vCPU);
  hash: the slot the key got, values + slot * S (host inserts into a fresh map take slots 0, 1, ...,
  emulator_linux_map_hash.go:56-64).
* A vCPU's packets run in order; map bytes carry over from packet to packet and from batch to batch
  of a VM; stack and xdp_md are fresh per process.
"""
from __future__ import annotations

import bisect
import functools
import os
import random
import re
import sys
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import opmatrix as OM  # noqa: E402  (the ALU / jump model)
from mimic_amd import asm as A  # noqa: E402

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
OK, UNRESOLVED, NOT_VMMEM, BOUNDS, NOT_DATASEC = 0, 3, 4, 5, 6      # include/mimic_amd.h

N_PACKETS = 1024
V_CPUS = 256
WAVE = 64
MEM_START = 0x10000           # memory_controller.go:55
STACK_SIZE = 2048             # StackFrameCount * StackFrameSize (vm.go:60-62)
FRAME = 256
XDP_MD_SIZE = 24
STK_FINE = 512                # runtime.h: a validity bit per word below, per granule above
GRANULE = 32                  # ... of 1 << chunk_shift bytes: 32 for a 2 KiB stack

# Byte alphabets, so that no store writes a byte that is already there: the packet's value field holds
# bytes 0x01..0x5f and the program stores it XOR VALUE_FLIP (0x81..0xdf: never the field's own bytes
# when the store lands on it); the constant-offset stores write 0xe1..0xe8, packet payload is 0xe0..0xfe,
# untouched memory is zero.  (Delta and xdp_md field bytes are arbitrary: batch() draws again.)
PREFILL = 0xE1E2E3E4E5E6E7E8
VALUE_FLIP = 0x8080808080808080
ST_IMM = -0x72839_4A6         # ST's constant: uint64 of it is 0xffffffff8d7c6b5a
FOLD_K = 0x01000193           # r0 = r0 * K + v: K odd, so any one changed v changes r0
SIZES = (1, 2, 4, 8)
OPS = ("ldx", "stx", "st")
assert ST_IMM & M32 == 0x8D7C6B5A


# ---------------------------------------------------------------------------------------------
# the model: the address space
# ---------------------------------------------------------------------------------------------
PLAIN, ARRAY_OBJ, OBJ = "plain", "array_obj", "obj"


class Entry:
    __slots__ = ("addr", "size", "kind", "mem", "map", "sub")

    def __init__(self, addr, size, kind, mem=None, map=None, sub=-1):
        self.addr, self.size, self.kind, self.mem, self.map, self.sub = addr, size, kind, mem, map, sub


class Space:
    """The static entries of one VM (maps, then programs, in API order) and, while a process runs,
    its stack, packet and xdp_md."""

    def __init__(self, vcpus: int, maps: List[dict], n_progs: int):
        self.vcpus = vcpus
        self.entries: List[Entry] = []
        self.next = MEM_START
        self.maps: Dict[str, dict] = {}
        for m in maps:
            self._add_map(m)
        self.prog_addr = [self._add(8, OBJ).addr for _ in range(n_progs)]
        self.starts = [e.addr for e in self.entries]
        self.static_next = self.next
        self.proc: Tuple[Entry, ...] = ()

    def _add(self, size, kind, mem=None, map=None, sub=-1) -> Entry:
        e = Entry(self.next, size, kind, mem, map, sub)     # nothing is ever freed below: first fit = append
        self.entries.append(e)
        self.next = e.addr + size + 1
        return e

    def _add_map(self, m):
        E, S, K, t = m["max_entries"], m["value_size"], m["key_size"], m["type"]
        st = dict(spec=m, values=[], slots={})
        if t == 2:        # LinuxArrayMap.Init, emulator_linux_map_array.go:30-54
            st["obj"] = self._add(8, ARRAY_OBJ, map=st)
            st["values"].append(self._add(E * S, PLAIN, bytearray(E * S)))
        elif t == 6:      # LinuxPerCPUArrayMap.Init :185-215
            st["obj"] = self._add(8, OBJ, map=st)
            for c in range(self.vcpus):
                self._add(8, ARRAY_OBJ, map=st, sub=c)
                st["values"].append(self._add(E * S, PLAIN, bytearray(E * S)))
        elif t == 1:      # LinuxHashMap.Init, emulator_linux_map_hash.go:43-97
            st["obj"] = self._add(8, OBJ, map=st)
            st["keys"] = self._add(E * K, PLAIN, bytearray(E * K))
            st["values"].append(self._add(E * S, PLAIN, bytearray(E * S)))
        else:
            raise ValueError(f"map type {t} is not in the corpus")
        self.maps[m["name"]] = st

    def _host_update(self, st, key: bytes, val: bytes):
        m = st["spec"]
        assert m["type"] == 1 and key not in st["slots"] and len(st["slots"]) < m["max_entries"]
        s = len(st["slots"])                               # the freelist pops 0, 1, ... in order
        st["slots"][bytes(key)] = s
        st["keys"].mem[s * m["key_size"]:(s + 1) * m["key_size"]] = key
        st["values"][0].mem[s * m["value_size"]:(s + 1) * m["value_size"]] = val

    # -- per process --------------------------------------------------------------------------
    def new_process(self, packet: bytes, H: int, T: int, idx=(0, 0, 0)):
        L = len(packet)
        St = self.static_next
        stack = Entry(St, STACK_SIZE, PLAIN, bytearray(STACK_SIZE))
        mem = bytearray(H + L + T)                         # the rooms are zero (context_xdp_md.go:52-64)
        mem[H:H + L] = packet
        pkt = Entry(St + STACK_SIZE + 1, H + L + T, PLAIN, mem)
        md = bytearray(XDP_MD_SIZE)
        for k, v in enumerate((pkt.addr + H, pkt.addr + H + L, pkt.addr + H) + tuple(idx)):
            md[4 * k:4 * k + 4] = (v & M32).to_bytes(4, "little")
        xdp = Entry(pkt.addr + pkt.size + 1, XDP_MD_SIZE, PLAIN, md)
        self.proc = (stack, pkt, xdp)
        return stack, pkt, xdp

    def get_entry(self, a: int) -> Optional[Entry]:
        """memory_controller.go:117-145"""
        if a >= self.static_next:
            for e in self.proc:
                if e.addr <= a <= e.addr + e.size:
                    return e
            return None
        i = bisect.bisect_right(self.starts, a) - 1
        if i >= 0:
            e = self.entries[i]
            if a <= e.addr + e.size:
                return e
        return None

    def access(self, a: int, n: int):
        """(status, entry, offset) of an n-byte LDX / STX / ST at address a (inst.go:298-363)."""
        e = self.get_entry(a)
        if e is None:
            return UNRESOLVED, None, 0
        if e.kind == OBJ:
            return NOT_VMMEM, None, 0
        if e.kind == ARRAY_OBJ:
            return NOT_DATASEC, None, 0                    # no map of the corpus is a datasec
        off = a - e.addr
        if off + n > len(e.mem):                           # memory_plain.go:27,57
            return BOUNDS, None, 0
        return OK, e, off

    def lookup(self, r1: int, r2: int, cpu: int) -> int:
        """bpf_map_lookup_elem for the calls the corpus makes (they cannot fail)."""
        e = self.get_entry(r1 & M32)
        assert e is not None and e.map is not None and e is e.map["obj"], "R1 is no map object of the corpus"
        st, m = e.map, e.map["spec"]
        s, ke, ko = self.access(r2 & M32, m["key_size"])
        assert s == OK
        key = bytes(ke.mem[ko:ko + m["key_size"]])
        if m["type"] == 1:
            slot = st["slots"].get(key)
            return 0 if slot is None else st["values"][0].addr + slot * m["value_size"]
        k = int.from_bytes(key, "little")
        if k >= m["max_entries"]:
            return 0
        return st["values"][cpu if m["type"] == 6 else 0].addr + k * m["value_size"]

    def map_values(self, name: str) -> List[bytes]:
        return [bytes(v.mem) for v in self.maps[name]["values"]]


# ---------------------------------------------------------------------------------------------
# the model: a process
# ---------------------------------------------------------------------------------------------
def decode(raw: bytes, relocs, space: Space):
    """[(op, dst, src, off, imm)]: LD_IMM64 slots with their 64-bit constant, a map reference
    rewritten to the map object's address (emulator_linux_.go:292-339), the second slot a Nop."""
    by_slot = dict(relocs)
    out = []
    n = len(raw) // 8
    i = 0
    while i < n:
        op, regs = raw[8 * i], raw[8 * i + 1]
        off = int.from_bytes(raw[8 * i + 2:8 * i + 4], "little", signed=True)
        imm = int.from_bytes(raw[8 * i + 4:8 * i + 8], "little", signed=True)
        if op == 0x18:
            v = (imm & M32) | (int.from_bytes(raw[8 * i + 12:8 * i + 16], "little") << 32)
            if i in by_slot:
                v = space.maps[by_slot[i]]["obj"].addr
            out += [(op, regs & 15, regs >> 4, off, v), (0, 0, 0, 0, 0)]
            i += 2
            continue
        out.append((op, regs & 15, regs >> 4, off, imm))
        i += 1
    return out


def run_process(space: Space, ins, packet: bytes, H=0, T=0, cpu=0, skip_pc=-1, stop_pc=-1):
    """Process.Run of one xdp_md process: (status, R0, steps, err_pc, packet memory).  skip_pc: the
    slot at that PC is stepped over as a Nop (the gate's counterfactual: one store left out).
    stop_pc: stop before that slot and return the registers (the process's memory stays in space.proc)."""
    stack, pkt, xdp = space.new_process(packet, H, T)
    r = [0] * 11
    r[1], r[10] = xdp.addr, stack.addr + FRAME
    pc = steps = 0
    n_ins = len(ins)
    access = space.access
    while True:
        assert 0 <= pc < n_ins
        if pc == stop_pc:
            return r
        op, dst, src, off, imm = ins[pc]
        steps += 1
        cls = op & 7
        if pc == skip_pc or op == 0:
            pc += 1
        elif cls == 1:                                    # LDX
            n = (4, 2, 1, 8)[(op >> 3) & 3]
            st, e, o = access((r[src] + off) & M32, n)
            if st:
                return st, r[0], steps, pc, bytes(pkt.mem)
            r[dst] = int.from_bytes(e.mem[o:o + n], "little")
            pc += 1
        elif cls == 3 or cls == 2:                        # STX / ST
            n = (4, 2, 1, 8)[(op >> 3) & 3]
            v = r[src] if cls == 3 else imm & M64         # uint64(Constant)
            st, e, o = access((r[dst] + off) & M32, n)
            if st:
                return st, r[0], steps, pc, bytes(pkt.mem)
            e.mem[o:o + n] = (v & ((1 << (8 * n)) - 1)).to_bytes(n, "little")
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
            return OK, r[0], steps, -1, bytes(pkt.mem)
        elif op == 0x85:
            assert imm == A.FN_MAP_LOOKUP_ELEM and src == 0
            r[0] = space.lookup(r[1], r[2], cpu)
            pc += 1
        else:
            what, v = OM.execute(op, imm, r[dst], r[src])
            if what == OM.SET:
                r[dst] = v
                pc += 1
            elif what == OM.JUMP:
                pc += 1 + (off if v else 0)
            else:
                raise ValueError(f"opcode {op:#x} is not in the corpus")


# ---------------------------------------------------------------------------------------------
# regions and programs
# ---------------------------------------------------------------------------------------------
MAPS = {
    "row24": dict(name="row24", type=6, key_size=4, value_size=8, max_entries=3),     # E * S = 24: register value cache
    "row72": dict(name="row72", type=6, key_size=4, value_size=8, max_entries=9),     # E * S = 72: LDS value cache
    "arr": dict(name="arr", type=2, key_size=4, value_size=16, max_entries=4),
    "hsh": dict(name="hsh", type=1, key_size=4, value_size=16, max_entries=4),
    "pad": dict(name="pad", type=2, key_size=4, value_size=8, max_entries=1),         # a neighbour above the last row
}
HASH_KEYS = (0x11, 0x22)
LOOKUP_KEY = {"row24": 0, "row72": 0, "arr": 1, "hsh": HASH_KEYS[1]}


def _init_bytes(tag: int, n: int) -> bytes:
    return bytes(0x30 + ((tag * 37 + 11 * k) % 0x60) for k in range(n))               # no byte zero


@dataclass(frozen=True)
class Region:
    name: str
    ops: Tuple[str, ...]
    map: str = ""             # the map whose lookup result is the base
    base_off: int = 0         # offset of the base inside its entry (the packet's: the headroom)
    backing: int = 0          # the entry's backing length B (the packet's: H + L + T)
    rand: Tuple[int, int] = (-64, 64)       # random offsets from rand[0] to B + rand[1]
    statuses: Tuple[int, ...] = ()          # every error status the region's neighbourhood can produce
    maps: Tuple[str, ...] = ()              # the maps its VM creates, in order
    ref: str = ""


REGIONS = (
    # below the stack lies the last program's object (not-VMMem), above it the packet
    Region("stack", OPS, base_off=FRAME, backing=STACK_SIZE, statuses=(BOUNDS, NOT_VMMEM), ref="vm.go:208-210"),
    # below the packet lies the stack's inclusive end, above it xdp_md (a store there lands) and then nothing
    Region("packet", OPS, rand=(-16, 40), statuses=(BOUNDS, UNRESOLVED), ref="context_xdp_md.go:52-64"),
    # nothing lies above xdp_md
    Region("xdp_md", OPS, backing=XDP_MD_SIZE, rand=(-8, 8), statuses=(BOUNDS, UNRESOLVED), ref="context_xdp_md.go:56-105"),
    # a row's neighbours: its sub-array's object below (under it the previous vCPU's inclusive end), the next
    # vCPU's object above.  No offset reaches another vCPU's row bytes: its lane runs at the same time
    Region("row24", OPS, map="row24", backing=24, rand=(-10, 9), statuses=(BOUNDS, NOT_DATASEC),
           maps=("row24", "pad"), ref="emulator_linux_map_array.go:185-241"),
    Region("row72", OPS, map="row72", backing=72, rand=(-10, 9), statuses=(BOUNDS, NOT_DATASEC),
           maps=("row72", "pad"), ref="emulator_linux_map_array.go:185-241"),
    Region("arr", ("ldx",), map="arr", base_off=16, backing=64, rand=(-24, 24), statuses=(BOUNDS, NOT_DATASEC, NOT_VMMEM),
           maps=("arr", "hsh"), ref="emulator_linux_map_array.go:78-94"),
    Region("hsh", ("ldx",), map="hsh", base_off=16, backing=64, rand=(-24, 24), statuses=(BOUNDS, NOT_VMMEM),
           maps=("arr", "hsh"), ref="emulator_linux_map_hash.go:134-155"),
)
REGION = {r.name: r for r in REGIONS}
# The VMs: one per (region, access), four programs (the sizes) each, so that every chunk owns the maps its
# forms need and no kernel takes long to compile (a kernel of twelve of these programs took hipRTC 165 s,
# the session prewarm's wall time is at least its longest kernel's); four programs have more slow-path
# sites than the JIT inlines, so every chunk kernel defers them
CHUNK_KEYS = tuple((R.name, op) for R in REGIONS for op in R.ops)


@functools.lru_cache(maxsize=None)
def lds_q() -> int:
    """MIMIC_LDS_STACK_Q of the kernels the JIT generates for programs that store through R10 (the
    LDS stack window covers the stack bytes [256 - 8 Q, 256)): read from the generated source."""
    from mimic_amd import jit as J

    raw = A.assemble([A.stx(8, 10, -8, 1), A.mov64_imm(0, 0), A.exit_()])[0]
    m = re.search(r"#define MIMIC_LDS_STACK_Q (\d+)", J.kernel_source([raw], 0))
    assert m, "the JIT no longer defines MIMIC_LDS_STACK_Q for a program that stores through R10"
    return int(m.group(1))


def window_lo() -> int:
    return FRAME - 8 * lds_q()


def stack_bounds() -> Tuple[int, ...]:
    """The stack's internal boundaries: the window's lower edge, R10, STK_FINE and the first two
    granule edges above it."""
    return window_lo(), FRAME, STK_FINE, STK_FINE + GRANULE, STK_FINE + 2 * GRANULE


def stack_readback() -> Tuple[int, ...]:
    """Stack offsets of the 8-byte words read back through R10: the word either side of every
    boundary (the edge offsets b - n .. b touch no other), the stack's first and last word, and the
    two words each straddling edge touches.  Every one is a site the kernel compiles a fast path and
    a slow path for, so no more than these."""
    W = window_lo()
    words = {0, STACK_SIZE - 8, W + 8, W + 16, STK_FINE + 8, STK_FINE + 16}
    for b in stack_bounds():
        words |= {b - 8, b}
    return tuple(sorted(words))


def stack_prefill() -> Tuple[Tuple[int, int], ...]:
    """(size, stack offset) of the constant-offset stores through R10: partly valid words either
    side of the window's lower edge and of STK_FINE, a whole word inside the window, the stack's
    first and last word."""
    W = window_lo()
    return ((2, W - 6), (1, W + 3), (8, W + 16), (2, 1), (1, STK_FINE + 5), (2, STK_FINE - 7), (2, STACK_SIZE - 3))


# (size, row offset) of the constant-offset stores through the lookup result: the whole row, in pieces, after
# the program folded what the vCPU's previous packet left there
ROW_PREFILL = {"row24": ((8, 0), (4, 8), (2, 12), (2, 14), (8, 16)),
               "row72": tuple((8, o) for o in range(0, 64, 8)) + ((4, 64), (4, 68))}
# the row's words folded before those stores and read back at the end (each a compiled site)
ROW_WORDS = {"row24": (0, 8, 16), "row72": (0, 8, 32, 56, 64)}


@dataclass(frozen=True)
class Form:
    region: str
    op: str
    n: int

    @property
    def name(self):
        return f"{self.region}_{self.op}{self.n}"

    @property
    def ref(self):
        return REGION[self.region].ref

    @property
    def rooms(self):
        """A third of the packet batches have per-packet head- and tailroom with dirty bytes."""
        return self.region == "packet" and (OPS.index(self.op) * 4 + SIZES.index(self.n)) % 3 == 1

    def _fold(self):
        return [A.alu64("mul", 0, FOLD_K), A.alu64("add", 0, 4, reg=True)]

    @functools.cached_property
    def items(self):
        R, n = REGION[self.region], self.n
        it = [A.mov64_reg(6, 1), A.ldx(4, 2, 6, 0), A.ldx(4, 3, 6, 4), A.mov64_reg(4, 2), A.alu64("add", 4, 16),
              A.jmp("jgt", 4, 3, "out", reg=True)]
        if R.map:
            it += [A.st(4, 10, -4, LOOKUP_KEY[R.map]), A.mov64_reg(2, 10), A.alu64("add", 2, -4), A.ld_map_fd(1, R.map),
                   A.call(A.FN_MAP_LOOKUP_ELEM), A.jmp("jeq", 0, 0, "out"), A.mov64_reg(1, 0), A.ldx(4, 2, 6, 0)]
        it += [A.ldx(4, 7, 2, 0), A.alu64("lsh", 7, 32), A.alu64("arsh", 7, 32), A.ldx(4, 9, 2, 4), A.alu64("lsh", 9, 32),
               A.alu64("add", 7, 9, reg=True), A.ldx(8, 8, 2, 8), A.ld_imm64(5, VALUE_FLIP), A.alu64("xor", 8, 5, reg=True), A.ld_imm64(5, PREFILL),
               A.mov64_reg(0, 8)]
        # constant-offset stores
        if self.region == "stack":
            it += [A.stx(k, 10, o - FRAME, 5) for k, o in stack_prefill()]
        else:
            it += [A.stx(8, 10, -(8 * lds_q() + 8), 5), A.stx(4, 10, -(8 * lds_q() - 4), 5)]     # either side of the edge
        if "stx" in R.ops and R.map:
            for o in ROW_WORDS[R.map]:                      # what the vCPU's previous packet left in the row
                it += [A.ldx(8, 4, 1, o)] + self._fold()
            it += [A.stx(k, 1, o, 5) for k, o in ROW_PREFILL[R.map]]
        # base + delta in a scratch register
        if self.region == "stack":
            it += [A.mov64_reg(9, 10)]
        elif self.region == "packet":
            it += [A.mov64_reg(9, 2)]
        elif self.region == "xdp_md":
            it += [A.mov64_reg(4, 1), A.mov64_reg(9, 4)]
        else:
            it += [A.mov64_reg(9, 1)]
        it += [A.alu64("add", 9, 7, reg=True), "access"]
        if self.op == "stx":
            it += [A.stx(n, 9, 0, 8)]
        elif self.op == "st":
            it += [A.st(n, 9, 0, ST_IMM)]
        it += [A.ldx(n, 4, 9, 0)] + self._fold()
        # read back at constant offsets
        if self.region == "stack":
            for o in stack_readback():
                it += [A.ldx(8, 4, 10, o - FRAME)] + self._fold()
        else:
            for o in (-(8 * lds_q() + 8), -(8 * lds_q())):
                it += [A.ldx(8, 4, 10, o)] + self._fold()
        for k, o in ((4, 0), (4, 4), (4, 8), (8, 10), (2, 22)) if self.region == "xdp_md" else ((4, 0), (4, 4)):
            it += [A.ldx(k, 4, 6, o)] + self._fold()
        for o in (0, 8):
            it += [A.ldx(8, 4, 2, o)] + self._fold()
        if R.map and "stx" in R.ops:
            for o in ROW_WORDS[R.map]:
                it += [A.ldx(8, 4, 1, o)] + self._fold()
        it += [A.exit_(), "out", A.mov64_imm(0, 2), A.exit_()]
        return it

    @functools.cached_property
    def asm(self):
        return A.assemble([x for x in self.items if x != "access"])

    @property
    def raw(self):
        return self.asm[0]

    @property
    def relocs(self):
        return self.asm[1]

    @functools.cached_property
    def access_pc(self) -> int:
        """The slot of the lane-varying access (a store form's store)."""
        pc = 0
        for x in self.items:
            if x == "access":
                return pc
            if not isinstance(x, str):
                pc += x.slots
        raise AssertionError


def _forms() -> List[Form]:
    return [Form(R.name, op, n) for R in REGIONS for op in R.ops for n in SIZES]


@functools.lru_cache(maxsize=None)
def forms() -> Tuple[Form, ...]:
    return tuple(_forms())


@functools.lru_cache(maxsize=None)
def chunks():
    """[(first form index, forms)]: one VM per (region, access)."""
    out = []
    for region, op in CHUNK_KEYS:
        idx = [k for k, f in enumerate(forms()) if (f.region, f.op) == (region, op)]
        assert idx == list(range(idx[0], idx[0] + 4))
        out.append((idx[0], [forms()[k] for k in idx]))
    return out


def one_per_region_op() -> List[int]:
    """One form per (region, op), the sizes rotating: 17 form indexes."""
    out, k = [], 0
    for R in REGIONS:
        for op in R.ops:
            out.append(forms().index(Form(R.name, op, SIZES[k % 4])))
            k += 1
    return out


def chunk_maps(fs) -> List[dict]:
    names = []
    for f in fs:
        for m in REGION[f.region].maps:
            if m not in names:
                names.append(m)
    return [MAPS[m] for m in names]


def scenario(fs):
    from harness import Scenario

    maps = chunk_maps(fs)
    init = []
    for m in maps:
        if m["name"] == "arr":
            init += [("arr", k.to_bytes(4, "little"), _init_bytes(k, 16), 0) for k in range(4)]
        if m["name"] == "hsh":
            init += [("hsh", k.to_bytes(4, "little"), _init_bytes(9 + j, 16), 0) for j, k in enumerate(HASH_KEYS)]
    return Scenario(vcpus=V_CPUS, maps=maps, progs=[(f"p{k}", f.raw, f.relocs) for k, f in enumerate(fs)], map_init=init)


def space_of(fs) -> Space:
    sc = scenario(fs)
    sp = Space(sc.vcpus, sc.maps, len(sc.progs))
    for name, key, val, _ in sc.map_init:
        st = sp.maps[name]
        if st["spec"]["type"] == 1:
            sp._host_update(st, key, val)
        else:                                              # LinuxArrayMap.Update, emulator_linux_map_array.go:97-113
            k, S = int.from_bytes(key, "little"), st["spec"]["value_size"]
            st["values"][0].mem[k * S:(k + 1) * S] = val
    return sp


# ---------------------------------------------------------------------------------------------
# deltas
# ---------------------------------------------------------------------------------------------
def edges(f: Form, H: int = 0, L: int = 16, T: int = 0) -> List[int]:
    """The edge offsets (inside the entry; delta = offset - base offset) of form f for a packet with
    rooms H, T and length L: around the start -1, 0, 1; around the end B - n, B - n + 1, B - 1, B
    (the inclusive end: resolves, then fails the bounds check) and B + 1 (the next entry's first
    byte, or nothing past xdp_md)."""
    R, n = REGION[f.region], f.n
    B = H + L + T if f.region == "packet" else R.backing
    out = [-1, 0, 1, B - n, B - n + 1, B - 1, B, B + 1]
    if f.region == "stack":
        for b in stack_bounds():
            out += [b - n, b - n + 1, b - 1, b]
        if n > 1:                                          # (o & 7) + n > 8 inside the window and outside it
            out += [window_lo() + 8 + 9 - n, STK_FINE + 8 + 9 - n]
        out += [-9, -10]                                   # the last program's first byte, the one before's last
    if f.region == "packet":                               # around data and data_end
        out += [H - 1, H, H + 1, H + L - n, H + L - n + 1, H + L - 1, H + L]
    if f.region in ("row24", "row72"):                     # the next vCPU's object [B + 1, B + 9]; this one's [-9, -1]
        out += [B + 2, B + 9, -9, -10]
    if f.region in ("arr", "hsh"):                         # the lookup's own value inside the backing
        out += [R.base_off - 1, R.base_off, R.base_off + 16 - n, -9, -10]
    return out


SEED = 0x3E3A7


def pack(d: int, hi: int, v: int) -> bytes:
    """A packet's first 16 bytes: the signed 32-bit delta, the bits 32..63 added to it, the value."""
    assert -(1 << 31) <= d < (1 << 31)
    return (d & M32).to_bytes(4, "little") + hi.to_bytes(4, "little") + v.to_bytes(8, "little")


def _store_rewrites_same_bytes(sp: Space, ins, f, pkt: bytes, H: int, T: int, cpu: int) -> bool:
    """Does the form's store land (by the model) on bytes that already hold what it writes?  Nothing
    could see such a store; batch() draws the packet's value (ST: its offset) again."""
    r = run_process(sp, ins, pkt, H, T, cpu, stop_pc=f.access_pc)
    st, e, o = sp.access(r[9] & M32, f.n)
    v = r[8] if f.op == "stx" else ST_IMM & M64
    return st == OK and bytes(e.mem[o:o + f.n]) == (v & ((1 << (8 * f.n)) - 1)).to_bytes(f.n, "little")


def _value(rng) -> int:
    return int.from_bytes(bytes(rng.randint(1, 0x5F) for _ in range(8)), "little")


@functools.lru_cache(maxsize=None)
def batch(index: int):
    """Form index's batch: dict(buf, off, lens, cpu, headroom, tailroom, delta, value, edge) with
    delta the signed offset from the base, bits 32..63 included, and value what an STX stores.  Even packets walk the form's edge
    list cyclically, odd packets draw an offset from region.rand around the entry; a quarter of the
    odd packets add random non-zero bits 32..63.  Nobody writes the arrays."""
    f = forms()[index]
    R = REGION[f.region]
    rng = random.Random(SEED * 131 + index)
    n = N_PACKETS
    if f.region == "packet":
        lens = [rng.choice((16, 17, 23, 24, 31, 60, 64, 65, 128, 590, 1500, 1514)) if rng.random() < 0.5 else rng.randint(16, 1514)
                for _ in range(n)]
    else:
        lens = [16] * n
    Hs = [rng.randint(0, 23) for _ in range(n)] if f.rooms else [0] * n
    Ts = [rng.randint(0, 16) for _ in range(n)] if f.rooms else [0] * n
    slot = [max(64, (Hs[k] + lens[k] + Ts[k] + 63) // 64 * 64) for k in range(n)]
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(slot)[:-1]
    nrng = np.random.default_rng(SEED + index)
    buf = nrng.integers(0, 256, int(sum(slot)), dtype=np.uint8)        # dirty room bytes: the run zeroes them
    if f.region == "packet":                               # payload bytes no store writes: 0xe0 .. 0xfe
        buf = (0xE0 + buf % 0x1F).astype(np.uint8)
    delta, value, edge = [], [], []
    n_edges = len(edges(f))
    fs = next(c[1] for c in chunks() if f in c[1])
    sp = space_of(fs)
    ins = decode(f.raw, f.relocs, sp)
    for k in range(n):
        H, L, T = Hs[k], lens[k], Ts[k]
        base = H if f.region == "packet" else R.base_off
        B = H + L + T if f.region == "packet" else R.backing
        d0 = int(off[k]) + H
        for attempt in range(64):
            hi = 0
            if k % 2 == 0:
                e = (k // 2) % n_edges
                d = edges(f, H, L, T)[e] - base
            else:
                e = -1
                d = rng.randint(R.rand[0], B + R.rand[1]) - base
                if rng.random() < 0.25:
                    hi = rng.randint(1, M32)
            v = _value(rng)
            buf[d0:d0 + 16] = np.frombuffer(pack(d, hi, v), np.uint8)
            if f.op == "ldx" or not _store_rewrites_same_bytes(sp, ins, f, bytes(buf[d0:d0 + L]), H, T, k % V_CPUS):
                break
        else:
            raise AssertionError(f"{f.name} packet {k}: every draw stores the bytes already there")
        edge.append(e)
        delta.append(d + (hi << 32))
        value.append(v ^ VALUE_FLIP)
    out = dict(buf=buf, off=off, lens=np.array(lens, np.uint32), cpu=(np.arange(n) % V_CPUS).astype(np.int32),
               headroom=np.array(Hs, np.uint32) if f.rooms else 0, tailroom=np.array(Ts, np.uint32) if f.rooms else 0,
               delta=np.array([d & M64 for d in delta], np.uint64), value=np.array(value, np.uint64),
               edge=np.array(edge, np.int32))
    for x in out.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return out


def runs(first: int, fs):
    out = []
    for k in range(len(fs)):
        b = batch(first + k)
        out.append(dict(entry=k, buf=b["buf"], off=b["off"], lens=b["lens"], cpu=b["cpu"], headroom=b["headroom"],
                        tailroom=b["tailroom"]))
    return out


def _rooms(b, k):
    H = b["headroom"] if np.isscalar(b["headroom"]) else int(b["headroom"][k])
    T = b["tailroom"] if np.isscalar(b["tailroom"]) else int(b["tailroom"][k])
    return int(H), int(T)


def model_sequence(first: int, fs, skip_store: bool = False):
    """The model's run of a chunk's sequence (one batch per form, on one address space): per form a
    dict of status / r0 / steps / err_pc arrays and the final packet buffer; then the final map
    bytes {name: [bytes per cpu]}.  skip_store: every packet runs with its lane-varying store left
    out, from the state the real run left for it (the gate's counterfactual), as
    out[k]["skip"] = [(r0, packet memory, the lane's map bytes) ...] next to the real ones in
    out[k]["real"]."""
    sp = space_of(fs)
    outs = []
    for j, f in enumerate(fs):
        b = batch(first + j)
        ins = decode(f.raw, f.relocs, sp)
        n = len(b["lens"])
        st, r0, steps, epc = np.zeros(n, np.int64), np.zeros(n, np.uint64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        buf = b["buf"].copy()
        real, skip = [], []
        names = [m["name"] for m in chunk_maps(fs) if m["type"] == 6]
        for k in range(n):
            H, T = _rooms(b, k)
            o, L, cpu = int(b["off"][k]), int(b["lens"][k]), int(b["cpu"][k])
            pkt = bytes(buf[o + H:o + H + L])
            if skip_store and f.op != "ldx":
                saved = {nm: bytes(sp.maps[nm]["values"][cpu].mem) for nm in names}
                s2 = run_process(sp, ins, pkt, H, T, cpu, skip_pc=f.access_pc)
                skip.append((s2[1], s2[4], {nm: bytes(sp.maps[nm]["values"][cpu].mem) for nm in names}))
                for nm in names:
                    sp.maps[nm]["values"][cpu].mem[:] = saved[nm]
            s = run_process(sp, ins, pkt, H, T, cpu)
            st[k], r0[k], steps[k], epc[k] = s[0], s[1], s[2], s[3]
            buf[o:o + H + L + T] = np.frombuffer(s[4], np.uint8)
            if skip_store and f.op != "ldx":
                real.append((s[1], s[4], {nm: bytes(sp.maps[nm]["values"][cpu].mem) for nm in names}))
        d = dict(status=st, r0=r0, steps=steps, err_pc=epc, pkt=buf)
        for x in d.values():
            x.setflags(write=False)
        if skip_store:
            d["real"], d["skip"] = real, skip
        outs.append(d)
    maps = {m["name"]: sp.map_values(m["name"]) for m in chunk_maps(fs)}
    return outs, maps


@functools.lru_cache(maxsize=None)
def expected(c: int):
    """The model's run of chunk c (computed once; read-only)."""
    first, fs = chunks()[c]
    return model_sequence(first, fs)


def assert_model(index: int, want, got, tag: str, check_pkt: bool = True):
    """got: a result dict of form index's batch against the model's `want`."""
    f = forms()[index]
    b = batch(index)
    for key in ("status", "r0", "steps", "err_pc"):
        g = np.asarray(got[key]).astype(np.uint64 if key == "r0" else np.int64)
        bad = np.nonzero(g != want[key])[0]
        if len(bad):
            k = int(bad[0])
            raise AssertionError(f"{tag} {f.name} ({f.ref}): {key} differs for {len(bad)} packets, first packet {k} "
                                 f"delta={int(b['delta'][k]):#x} edge={int(b['edge'][k])} len={int(b['lens'][k])}: "
                                 f"got {int(g[k]):#x} model {int(want[key][k]):#x} (model status {int(want['status'][k])})")
    if check_pkt:
        g = np.asarray(got["pkt"])
        bad = np.nonzero(g[:len(want["pkt"])] != want["pkt"][:len(g)])[0]
        if len(bad):
            k = int(np.searchsorted(b["off"], bad[0], side="right")) - 1
            raise AssertionError(f"{tag} {f.name}: packet memory differs at byte {int(bad[0])} (packet {k}, "
                                 f"delta={int(b['delta'][k]):#x})")


def assert_model_maps(want_maps, got_maps, tag: str):
    for name, vals in want_maps.items():
        for c, v in enumerate(vals):
            assert bytes(got_maps[name][c]) == v, f"{tag}: map {name} cpu {c} differs from the model"


# Process.Run: the edge list first, then random offsets around the entry, 32 in all
def proc_cases(index: int):
    """[(packet bytes, cpu)] of 32 single processes for form index: no rooms, 16-byte packets (the
    packet region: 64 bytes), four vCPUs so that rows carry over from process to process."""
    f = forms()[index]
    R = REGION[f.region]
    L = 64 if f.region == "packet" else 16
    B = L if f.region == "packet" else R.backing
    ds = [e - R.base_off for e in edges(f, 0, L, 0)]
    rng = random.Random(SEED + 7 * index)
    while len(ds) < 32:
        ds.append(rng.randint(R.rand[0], B + R.rand[1]) - R.base_off)
    out = []
    for j, d in enumerate(ds[:32]):
        hi = rng.randint(1, M32) if j % 8 == 7 else 0
        out.append((pack(d, hi, _value(rng)) + bytes(range(1, L - 15)), j % 4))
    return out


# ---------------------------------------------------------------------------------------------
# sk_buff: LDX / STX through __sk_buff's data pointer plus a lane-varying delta, against the oracle
# only (the per-process entries earlier processes leaked move every address from packet to packet:
# no model).  Packet memory is big endian there (emulator_linux_sk_buff.go:108-121): the frame-only
# fast store against the generic store in the rooms.
# ---------------------------------------------------------------------------------------------
SKB_H, SKB_T = 32, 64          # SKBuffFromBytes' headroom and tailroom
SKB_AT = 48                    # frame offset of the 16 bytes (delta, bits 32..63, value): inside every IMIX frame


@dataclass(frozen=True)
class SkbForm:
    op: str
    n: int

    @property
    def name(self):
        return f"skb_{self.op}{self.n}"

    @functools.cached_property
    def raw(self):
        fold = [A.alu64("mul", 0, FOLD_K), A.alu64("add", 0, 4, reg=True)]
        it = [A.mov64_reg(6, 1), A.ldx(4, 2, 6, A.SKB["data"]), A.ldx(4, 3, 6, A.SKB["data_end"]), A.mov64_reg(4, 2),
              A.alu64("add", 4, SKB_AT + 16), A.jmp("jgt", 4, 3, "out", reg=True),
              A.ldx(4, 7, 2, SKB_AT), A.alu64("lsh", 7, 32), A.alu64("arsh", 7, 32), A.ldx(4, 9, 2, SKB_AT + 4),
              A.alu64("lsh", 9, 32), A.alu64("add", 7, 9, reg=True), A.ldx(8, 8, 2, SKB_AT + 8), A.mov64_reg(0, 8),
              A.mov64_reg(9, 2), A.alu64("add", 9, 7, reg=True)]
        if self.op == "stx":
            it += [A.stx(self.n, 9, 0, 8)]
        it += [A.ldx(self.n, 4, 9, 0)] + fold
        for k, o in ((8, 0), (8, SKB_AT), (8, SKB_AT + 8)):
            it += [A.ldx(k, 4, 2, o)] + fold
        for fld in ("data", "data_end", "len"):
            it += [A.ldx(4, 4, 6, A.SKB[fld])] + fold
        it += [A.exit_(), "out", A.mov64_imm(0, 2), A.exit_()]
        return A.assemble(it)[0]


SKB_FORMS = tuple(SkbForm(op, n) for op in ("ldx", "stx") for n in SIZES)


def skb_scenario():
    from harness import Scenario

    return Scenario(vcpus=V_CPUS, progs=[(f.name, f.raw, []) for f in SKB_FORMS])


def skb_edges(n: int, L: int) -> List[int]:
    """Offsets from data: around the headroom's start, data, data_end and the tailroom's end."""
    return [-SKB_H - 1, -SKB_H, -SKB_H + 1, -n, -n + 1, -1, 0, 1, L - n, L - n + 1, L - 1, L, L + SKB_T - n,
            L + SKB_T - n + 1, L + SKB_T - 1, L + SKB_T, L + SKB_T + 1]


@functools.lru_cache(maxsize=None)
def skb_batch(index: int):
    """IMIX frames (mimic_amd.workloads) with the 16 bytes at SKB_AT rewritten, big endian: even
    packets walk skb_edges, odd packets draw an offset from 8 bytes below the headroom to 8 past
    the tailroom, a quarter of them with bits 32..63."""
    from mimic_amd import workloads as W

    f = SKB_FORMS[index]
    buf, off, lens = W.make_skb_packets(N_PACKETS, **W.IMIX, seed=SEED + index)
    buf = np.array(buf, np.uint8)
    rng = random.Random(SEED * 7 + index)
    for k in range(N_PACKETS):
        L = int(lens[k])
        hi = 0
        if k % 2 == 0:
            e = skb_edges(f.n, L)
            d = e[(k // 2) % len(e)]
        else:
            d = rng.randint(-SKB_H - 8, L + SKB_T + 8)
            if rng.random() < 0.25:
                hi = rng.randint(1, M32)
        at = int(off[k]) + SKB_H + SKB_AT
        buf[at:at + 16] = np.frombuffer((d & M32).to_bytes(4, "big") + hi.to_bytes(4, "big") + _value(rng).to_bytes(8, "big"),
                                        np.uint8)
    cpu = (np.arange(N_PACKETS) % V_CPUS).astype(np.int32)
    for x in (buf, off, lens, cpu):
        x.setflags(write=False)
    return dict(skb=True, entry=index, buf=buf, off=np.asarray(off, np.uint64), lens=np.asarray(lens, np.uint32), cpu=cpu)


def skb_runs():
    return [skb_batch(k) for k in range(len(SKB_FORMS))]
