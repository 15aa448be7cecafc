"""Map helpers and tail calls over per-packet arguments: a model of the helpers and a corpus.

The helper KATs (tests/golden/make_golden.py, "maps" / "tail calls" / "hash maps") run one packet per
batch and build every argument with LD_IMM64, MOV imm or r10 + const; the workloads and fuzz_struct.py
vary the key bytes per lane but never the map pointer, the key pointer, the value pointer or the
tail-call index.  Here every program takes one argument of one helper call from the packet, in the
shape of tests/memmatrix.py:

    r6 = r1; r2 = data; r3 = data_end; if (r2 + 16 > r3) goto out
    r7 = (s64)*(s32 *)(r2 + 0) + ((u64)*(u32 *)(r2 + 4) << 32)      the delta, bits 32..63 apart
    r8 = *(u64 *)(r2 + 8); r0 = r8                                    never zero: a failing call keeps it
    constant stores (the 40-byte key PAT at r10 - 40, an update's value at r10 - 64, ...)
    r9 = base; r9 += r7                                               the lane-varying argument
    r1 .. r5 = the arguments (all set, R4 = flags = r8: every map's Update ignores them)
    call                                                              the lane-varying call
    r9 = r0; r0 = r8; r0 = r0 * K + r9                                the helper's R0 (FOLD_K)
    a non-zero lookup result: *(u64 *)(r9 + 0), *(u32 *)(r9 + 8) folded
    R1 .. R5 folded (helpers keep them, Q8; cold_* hands them through a Spill record)
    a constant-argument lookup of every map the call may have changed, its bytes folded
    call 8 (bpf_get_smp_processor_id) folded; exit                    (out: r0 = 2; exit)

over N_PACKETS packets on V_CPUS vCPUs with cpu[k] = k % V_CPUS, so the 64 lanes of a wave hold 64
consecutive packets: one lane's R1 names the per-CPU array's object, its neighbour's another CPU's
sub-array object, the next one a hash map through a double pointer on the stack, the next one fails
with MIMIC_ERR_HELPER_MAP_PTR beside lanes that go on and read the value back.

Every VM holds the same eight maps (MAPS: a plain array, per-CPU arrays with a 24- and a 72-byte row,
hash maps with a 20- and a 40-byte key, a per-CPU hash, a prog array, a plain array with four entries
per vCPU), the chunk's programs and three tail-call targets (two that fold different constants and an
empty one).

The model restates the reference in Python integers, bytearrays and dicts on memmatrix.Space (the
address space; its docstring has MemoryController / PlainMemory / LDX / STX):

* regToMap (emulator_linux_helpers.go:415-447): GetEntry(uint32(reg)); a LinuxMap object (a map's
  object, or a per-CPU array's sub-array object, which is a LinuxArrayMap of that CPU whatever the
  process's CPU, emulator_linux_map_array.go:202-208) is the map; any other VMMem is read as a
  double pointer: Load(off, Word) (off + 4 > len fails), GetEntry of that word, which must be a
  LinuxMap; everything else is an error (MIMIC_ERR_HELPER_MAP_PTR).
* derefMapKey (:449-471) and the value deref (:525-541): GetEntry(uint32(reg)), a VMMem, Read of
  key-size / value-size bytes: off + n > len fails, so does a non-datasec array object
  (MIMIC_ERR_HELPER_KEY / MIMIC_ERR_HELPER_VALUE).
* bpf_map_lookup_elem / update_elem / delete_elem (:477-586): map, then key, then value; delete
  asks for a LinuxMapDeleter before it reads the key (:565-568: arrays are none,
  MIMIC_ERR_HELPER_MAP_OP); a syscall.Errno goes to R0 as uint64(errno): E2BIG is 7; R4 is ignored.
* LinuxArrayMap / LinuxPerCPUArrayMap (emulator_linux_map_array.go:78-113, 235-250): the key is a
  native-endian uint32; Lookup of key >= MaxEntries is 0, Update E2BIG; the per-CPU map uses the
  process's CPU (its cpuid errors cannot happen: every process has a vCPU of the VM); Update writes
  a copy of the value bytes (memmove when source and destination overlap).
* LinuxHashMap / LinuxPerCPUHashMap (emulator_linux_map_hash.go:134-255, 537-664): KeyToIndex, a
  FIFO freelist 0 .. E-1; Update of a new key pops the head (empty: E2BIG), writes key and value
  (per-CPU: the process's CPU's value only); Delete of an absent key is nil, of a present one pushes
  its slot to the tail.  Per-CPU hash layout: V values backings, the object, the keys (:439-500).
* bpf_tail_call (:649-738): the budget check first (pastTailcalls >= MaxTailCalls: R0 = -EPERM); R2
  through regToMap; not a ProgramArray with 4-byte keys: an error (MIMIC_ERR_HELPER_TAILCALL); the
  key is uint32(R3); Lookup's address through GetEntry (not found -- key out of range gives address
  0 -- : R0 = -EINVAL); the word loaded there (a load error is ignored, :707-710) through GetEntry:
  not found: -EINVAL, no program: -EINVAL; else the process continues at PC 0 of that program with
  every register kept; an empty program ends it with errInvalidProgramCount at the call's PC
  (vm.go:327-334).
* bpf_get_smp_processor_id (:603-606): R0 = the process's CPU.
* bpf_xdp_adjust_tail up to its 20-byte check (:842-864): GetEntry(uint32(R1)) not found, no
  *PlainMemory, or a backing that is not 20 bytes long: R0 = -EINVAL.  Past that check the engine
  reports MIMIC_ERR_ENGINE_HELPER (as KAT helper_ktime_engine does for helper 5).
* A failing call counts as a step and leaves the registers as they were (vm.go:291-340).

Delete with a lane-varying MAP pointer: lanes that name an array fail with MIMIC_ERR_HELPER_MAP_OP
beside lanes that name a hash map.  hashmap.h's wave-cooperative insert and delete (h_insert_wave,
h_insert_nolock, h_delete_wave) reserve freelist positions once per round for all their lanes on the
table of the round's first lane (the open finding), so the lanes that FREE or TAKE a
slot in one call must name one table: the form's key (the vCPU's own, generation 2) is held by h20
alone, and a delete of an absent key in h40 or the per-CPU hash touches no freelist.
Left out for the same reason: update with a lane-varying map pointer (its lanes would insert into
three tables at once; and 256 vCPUs would write the plain array's six entries).  The index update on
a plain array runs on `arrv` (E = 4 V): in range a lane names only its vCPU's own four entries.

Concurrency (the GPU runs the vCPUs side by side): the forms that mutate a shared hash map take
their key from packets whose bytes are random per packet with the vCPU in the key the form aims at,
fold `r0 != 0` and the bytes behind it (never a hash address), and their final maps compare by key;
the plain array `arrv` is written at 4 * cpu + j only; test_helpmatrix_cpu.py asserts it on the
model's touch log.
"""
from __future__ import annotations

import functools
import os
import random
import sys
from collections import deque
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import memmatrix as MM  # noqa: E402  (the address space)
import opmatrix as OM  # noqa: E402  (the ALU / jump model)
from mimic_amd import asm as A  # noqa: E402

M64, M32 = MM.M64, MM.M32
OK, PC_OOB, UNRESOLVED, BOUNDS = 0, 1, 3, 5                                   # include/mimic_amd.h
MAP_PTR, KEY, VALUE, MAP_OP, TAILCALL, ENGINE_HELPER = 8, 9, 10, 11, 12, 24
E2BIG, EPERM, EINVAL = 7, (-1) & M64, (-22) & M64
N_PACKETS, V_CPUS, WAVE = MM.N_PACKETS, MM.V_CPUS, MM.WAVE
FRAME, STACK_SIZE, XDP_MD_SIZE = MM.FRAME, MM.STACK_SIZE, MM.XDP_MD_SIZE
FOLD_K, PREFILL = MM.FOLD_K, MM.PREFILL
MAX_TAIL = 33                                                                # LinuxEmulator's default MaxTailCalls
SEED = 0x4E1F7

# the 40 bytes at r10 - 40: index 0 for the arrays, then no byte zero; its prefixes are hash keys
PAT = bytes(4) + bytes(0x41 + k for k in range(36))

MAPS = (
    dict(name="arr", type=2, key_size=4, value_size=12, max_entries=6),      # the first entry: its object is at 0x10000
    dict(name="pc24", type=6, key_size=4, value_size=24, max_entries=1),     # a 24-byte row (register value cache)
    dict(name="pc72", type=6, key_size=4, value_size=12, max_entries=6),     # a 72-byte row; 12: a partial last chunk
    dict(name="h20", type=1, key_size=20, value_size=12, max_entries=4096),  # the inline probe (key <= 32)
    dict(name="h40", type=1, key_size=40, value_size=16, max_entries=8),     # generic only
    dict(name="ph", type=5, key_size=8, value_size=12, max_entries=2048),
    dict(name="progs", type=3, key_size=4, value_size=4, max_entries=10),
    dict(name="arrv", type=2, key_size=4, value_size=12, max_entries=4 * V_CPUS),   # a plain array updated at index 4 * cpu + j
)
SPEC = {m["name"]: m for m in MAPS}
ARRAYS, HASHES = (2, 3, 6), (1, 5)
T_CONST = (0x7A01, 0x7B02)                                                   # what the two targets fold
N_TARGETS = 3                                                                # t0, t1, empty
SELF_SLOT = 8                                                                # the prog array slot of the budget form


# ---------------------------------------------------------------------------------------------
# the model: the maps on the address space
# ---------------------------------------------------------------------------------------------
class Space(MM.Space):
    """memmatrix.Space with prog arrays, per-CPU hashes, the hash freelist and the helpers."""

    def __init__(self, vcpus, maps, n_progs):
        super().__init__(vcpus, maps, n_progs)
        self.prog_index = {a: k for k, a in enumerate(self.prog_addr)}
        self.log = None                                    # [(map, key, cpu)] of a mutating form's shared-map touches
        self.last_map = None                               # the map regToMap found last

    def _add_map(self, m):
        E, S, K, t = m["max_entries"], m["value_size"], m["key_size"], m["type"]
        if t == 3:        # a ProgramArray is a LinuxArrayMap (emulator_linux_map_array.go:30-54)
            st = dict(spec=m, values=[], slots={})
            st["obj"] = self._add(8, MM.ARRAY_OBJ, map=st)
            st["values"].append(self._add(E * S, MM.PLAIN, bytearray(E * S)))
            self.maps[m["name"]] = st
        elif t == 5:      # LinuxPerCPUHashMap.Init, emulator_linux_map_hash.go:439-500
            st = dict(spec=m, values=[], slots={})
            for _ in range(self.vcpus):
                st["values"].append(self._add(E * S, MM.PLAIN, bytearray(E * S)))
            st["obj"] = self._add(8, MM.OBJ, map=st)
            st["keys"] = self._add(E * K, MM.PLAIN, bytearray(E * K))
            self.maps[m["name"]] = st
        else:
            super()._add_map(m)
        if t in HASHES:
            self.maps[m["name"]]["free"] = deque(range(E))   # emulator_linux_map_hash.go:61-64

    # -- emulator_linux_helpers.go:415-447 -------------------------------------------------------
    def reg_to_map(self, reg: int):
        e = self.get_entry(reg & M32)
        if e is None:
            return None
        if e.map is not None:
            self.last_map = e.map["spec"]["name"]
            return e.map, e.sub
        if e.kind != MM.PLAIN:                             # a program: no LinuxMap, no VMMem
            return None
        off = (reg & M32) - e.addr
        if off + 4 > len(e.mem):
            return None
        e2 = self.get_entry(int.from_bytes(e.mem[off:off + 4], "little"))
        if e2 is None or e2.map is None:
            return None
        self.last_map = e2.map["spec"]["name"]
        return e2.map, e2.sub

    def read(self, reg: int, n: int):
        """derefMapKey / the value deref: n bytes, or None."""
        s, e, o = self.access(reg & M32, n)
        return bytes(e.mem[o:o + n]) if s == OK else None

    def _touch(self, st, key, cpu):
        if self.log is not None and st["spec"]["type"] in (1, 2, 5):
            if st["spec"]["type"] == 2 and int.from_bytes(key, "little") >= st["spec"]["max_entries"]:
                return                                     # no entry of the array: Lookup is 0, Update E2BIG
            self.log.append((st["spec"]["name"], bytes(key), cpu))

    def lookup(self, st, sub, key: bytes, cpu: int) -> int:
        m = st["spec"]
        self._touch(st, key, cpu)
        if m["type"] in ARRAYS:
            k = int.from_bytes(key, "little")
            if k >= m["max_entries"]:
                return 0
            which = (cpu if sub < 0 else sub) if m["type"] == 6 else 0
            return st["values"][which].addr + k * m["value_size"]
        slot = st["slots"].get(key)
        if slot is None:
            return 0
        return st["values"][cpu if m["type"] == 5 else 0].addr + slot * m["value_size"]

    def update(self, st, sub, key: bytes, val: bytes, cpu: int) -> int:
        m = st["spec"]
        S = m["value_size"]
        self._touch(st, key, cpu)
        if m["type"] in ARRAYS:
            k = int.from_bytes(key, "little")
            if k >= m["max_entries"]:
                return E2BIG
            which = (cpu if sub < 0 else sub) if m["type"] == 6 else 0
            st["values"][which].mem[k * S:(k + 1) * S] = val
            return 0
        slot = st["slots"].get(key)
        if slot is None:
            if not st["free"]:
                return E2BIG
            slot = st["free"].popleft()
            st["slots"][key] = slot
        K = m["key_size"]
        st["keys"].mem[slot * K:(slot + 1) * K] = key
        st["values"][cpu if m["type"] == 5 else 0].mem[slot * S:(slot + 1) * S] = val
        return 0

    def delete(self, st, key: bytes, cpu: int) -> int:
        self._touch(st, key, cpu)
        slot = st["slots"].pop(key, None)
        if slot is not None:
            st["free"].append(slot)                        # emulator_linux_map_hash.go:247-252
        return 0

    def hash_contents(self, name):
        st = self.maps[name]
        S = st["spec"]["value_size"]
        return {k: [bytes(v.mem[s * S:(s + 1) * S]) for v in st["values"]] for k, s in st["slots"].items()}


def run_process(sp: Space, progs, entry: int, packet: bytes, H=0, T=0, cpu=0, skip_pc=-1, max_tail=MAX_TAIL, call_pc=-1):
    """Process.Run of one xdp_md process that starts in progs[entry] (decoded programs of the VM in
    load order): (status, R0, steps, err_pc, packet memory, the program it ended in, what the call
    at call_pc of the entry program did last: R0 after it, 2^64 + the program a tail call went to, or
    minus the status it failed with).  skip_pc: that slot of the entry program is stepped over as a
    Nop (the gate's counterfactual)."""
    stack, pkt, xdp = sp.new_process(packet, H, T)
    r = [0] * 11
    r[1], r[10] = xdp.addr, stack.addr + FRAME
    cur, ins = entry, progs[entry]
    pc = steps = tails = 0
    access = sp.access
    outcome = None
    at_call = False

    def end(st, epc):
        o = outcome
        if st and cur == entry and epc == call_pc:
            o = -st
        return st, r[0], steps, epc, bytes(pkt.mem), cur, o

    while True:
        if at_call:                                       # the call at call_pc returned
            outcome, at_call = r[0], False
        op, dst, src, off, imm = ins[pc]
        steps += 1
        cls = op & 7
        at_call = cur == entry and pc == call_pc and op == 0x85
        if op == 0 or (pc == skip_pc and tails == 0):
            pc += 1
        elif cls == 1:                                    # LDX
            n = (4, 2, 1, 8)[(op >> 3) & 3]
            st, e, o = access((r[src] + off) & M32, n)
            if st:
                return end(st, pc)
            r[dst] = int.from_bytes(e.mem[o:o + n], "little")
            pc += 1
        elif cls == 3 or cls == 2:                        # STX / ST
            n = (4, 2, 1, 8)[(op >> 3) & 3]
            v = r[src] if cls == 3 else imm & M64
            st, e, o = access((r[dst] + off) & M32, n)
            if st:
                return end(st, pc)
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
            return end(OK, -1)
        elif op == 0x85 and imm in (A.FN_MAP_LOOKUP_ELEM, A.FN_MAP_UPDATE_ELEM, A.FN_MAP_DELETE_ELEM):
            m = sp.reg_to_map(r[1])
            if m is None:
                return end(MAP_PTR, pc)
            st_, sub = m
            spec = st_["spec"]
            if imm == A.FN_MAP_DELETE_ELEM and spec["type"] in ARRAYS:       # :565-568, before the key
                return end(MAP_OP, pc)
            key = sp.read(r[2], spec["key_size"])
            if key is None:
                return end(KEY, pc)
            if imm == A.FN_MAP_LOOKUP_ELEM:
                r[0] = sp.lookup(st_, sub, key, cpu)
            elif imm == A.FN_MAP_DELETE_ELEM:
                r[0] = sp.delete(st_, key, cpu)
            else:
                val = sp.read(r[3], spec["value_size"])
                if val is None:
                    return end(VALUE, pc)
                r[0] = sp.update(st_, sub, key, val, cpu)
            pc += 1
        elif op == 0x85 and imm == A.FN_GET_SMP_PROCESSOR_ID:
            r[0] = cpu
            pc += 1
        elif op == 0x85 and imm == A.FN_TAIL_CALL:
            if tails >= max_tail:                         # :663-666, before anything else
                r[0] = EPERM
                pc += 1
                continue
            m = sp.reg_to_map(r[2])
            if m is None:
                return end(MAP_PTR, pc)
            st_, sub = m
            if st_["spec"]["type"] != 3 or st_["spec"]["key_size"] != 4:     # :674-681
                return end(TAILCALL, pc)
            a = sp.lookup(st_, -1, (r[3] & M32).to_bytes(4, "little"), cpu)
            e = sp.get_entry(a)
            target = None
            if e is not None:                             # (not found: -EINVAL, :694-699)
                if e.kind == MM.OBJ:                      # no VMMem (:701-704; a prog array's values are)
                    return end(TAILCALL, pc)
                o = a - e.addr
                pa = int.from_bytes(e.mem[o:o + 4], "little") if e.kind == MM.PLAIN and o + 4 <= len(e.mem) else 0
                e2 = sp.get_entry(pa)
                if e2 is not None and e2.addr in sp.prog_index and e2.kind == MM.OBJ and e2.map is None:
                    target = sp.prog_index[e2.addr]
            if target is None:
                r[0] = EINVAL
                pc += 1
                continue
            if at_call:
                outcome, at_call = (1 << 64) + target, False
            cur, ins = target, progs[target]
            tails += 1
            if not ins:                                   # vm.go:327-334 after PC = -1
                return end(PC_OOB, pc)
            pc = 0
        elif op == 0x85 and imm == A.FN_XDP_ADJUST_TAIL:  # :842-864
            e = sp.get_entry(r[1] & M32)
            if e is None or e.kind != MM.PLAIN or len(e.mem) != 20:
                r[0] = EINVAL
                pc += 1
            else:
                return end(ENGINE_HELPER, pc)
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
# programs
# ---------------------------------------------------------------------------------------------
def _fold(x):
    return [A.alu64("mul", 0, FOLD_K), A.alu64("add", 0, x, reg=True)]


def _prologue(need=16):
    return [A.mov64_reg(6, 1), A.ldx(4, 2, 6, 0), A.ldx(4, 3, 6, 4), A.mov64_reg(4, 2), A.alu64("add", 4, need),
            A.jmp("jgt", 4, 3, "out", reg=True),
            A.ldx(4, 7, 2, 0), A.alu64("lsh", 7, 32), A.alu64("arsh", 7, 32), A.ldx(4, 9, 2, 4), A.alu64("lsh", 9, 32),
            A.alu64("add", 7, 9, reg=True), A.ldx(8, 8, 2, 8), A.mov64_reg(0, 8)]


def _store_bytes(reg, off, data: bytes):
    assert len(data) % 4 == 0
    return [A.st(4, reg, off + k, int.from_bytes(data[k:k + 4], "little")) for k in range(0, len(data), 4)]


def _after(deref: bool, noaddr: bool, tag: str):
    """After a call: the helper's R0 into the fold (r8 holds the fold so far), then the bytes behind
    a lookup result.  noaddr: `r0 != 0` in place of the address."""
    it = [A.mov64_reg(9, 0), A.mov64_reg(0, 8)]
    if noaddr:
        it += [A.mov64_imm(7, 1), A.jmp("jne", 9, 0, tag + "n"), A.mov64_imm(7, 0), tag + "n"] + _fold(7)
    else:
        it += _fold(9)
    if deref:
        it += [A.jmp("jeq", 9, 0, tag + "z"), A.ldx(8, 7, 9, 0)] + _fold(7) + [A.ldx(4, 7, 9, 8)] + _fold(7) + [tag + "z"]
    return it


def _readback(map_name: str, key_items, words: int, tag: str, noaddr=False):
    """A constant-argument lookup and `words` 8-byte words (the last one 4 bytes where the value ends
    in half a word) behind its result, folded."""
    S = SPEC[map_name]["value_size"]
    it = [A.mov64_reg(8, 0)] + key_items + [A.ld_map_fd(1, map_name), A.call(A.FN_MAP_LOOKUP_ELEM)]
    it += _after(False, noaddr, tag)
    it += [A.jmp("jeq", 9, 0, tag + "e")]
    total = words * 8 if words else S
    for o in range(0, total, 8):
        it += [A.ldx(8 if total - o >= 8 else 4, 7, 9, o)] + _fold(7)
    return it + [tag + "e"]


KEY_AT = -104                                            # the constant keys of the read-backs


def _const_key(k: int):
    return [A.st(4, 10, KEY_AT, k), A.mov64_reg(2, 10), A.alu64("add", 2, KEY_AT)]


@dataclass(frozen=True)
class Form:
    kind: str                 # mapptr | key | val | idx | budget | adjtail
    op: str = "lookup"        # lookup | update | delete | tail
    region: str = ""          # stack | packet | xdp | row | own
    map: str = ""

    @property
    def name(self):
        return "_".join(x for x in (self.kind, self.region, self.map, self.op) if x)

    @property
    def group(self) -> int:
        return ("mapptr", "key", "val", "idx", "budget", "adjtail").index(self.kind) + 1

    @property
    def ref(self):
        return {"lookup": "emulator_linux_helpers.go:477-504", "update": "emulator_linux_helpers.go:506-555",
                "delete": "emulator_linux_helpers.go:557-586", "tail": "emulator_linux_helpers.go:649-738",
                "adjust": "emulator_linux_helpers.go:842-864"}[self.op]

    @property
    def mutates_hash(self) -> bool:
        if self.kind == "mapptr":                          # whatever map the lane names: the hash maps among them
            return self.op == "delete"
        return self.op in ("update", "delete") and SPEC.get(self.map, {}).get("type") in HASHES

    @property
    def mutating(self) -> bool:
        return self.op in ("update", "delete")

    @property
    def rooms(self) -> bool:
        """Per-packet head- and tailroom with dirty bytes for two of the packet-region forms."""
        return self.region == "packet" and self.map in ("arr", "pc24") and self.op in ("lookup", "update")

    @property
    def size(self) -> int:
        """Bytes read through the lane-varying pointer."""
        if self.kind == "key":
            return SPEC[self.map]["key_size"]
        if self.kind == "val":
            return SPEC[self.map]["value_size"]
        return 0

    @property
    def statuses(self) -> Tuple[int, ...]:
        """Every error status the form's corpus must produce in every batch."""
        return {"mapptr": {"tail": (MAP_PTR, TAILCALL), "delete": (MAP_PTR, MAP_OP)}.get(self.op, (MAP_PTR,)), "key": (KEY,), "val": (VALUE,),
                "idx": (PC_OOB,) if self.op == "tail" else (), "budget": (), "adjtail": (ENGINE_HELPER,)}[self.kind]

    @property
    def errnos(self) -> Tuple[int, ...]:
        """Every R0 errno the lane-varying call must return in every batch."""
        if self.kind == "idx":
            return {"tail": (EINVAL,), "update": (E2BIG,)}.get(self.op, ())
        return {"budget": (EPERM,), "adjtail": (EINVAL,)}.get(self.kind, ())

    @functools.cached_property
    def items(self):
        k, op, region, mp = self.kind, self.op, self.region, self.map
        fn = {"lookup": A.FN_MAP_LOOKUP_ELEM, "update": A.FN_MAP_UPDATE_ELEM, "delete": A.FN_MAP_DELETE_ELEM,
              "tail": A.FN_TAIL_CALL, "adjust": A.FN_XDP_ADJUST_TAIL}[op]
        noaddr = self.mutates_hash
        if k == "budget":
            it = [A.jmp("jne", 6, 0, "loop")] + _prologue() + ["loop", A.jmp("jeq", 7, 0, "done"), A.alu64("add", 7, -1)]
            it += _fold(7) + [A.mov64_reg(1, 6), A.ld_map_fd(2, "progs"), A.mov64_imm(3, SELF_SLOT), "call", A.call(fn)]
            it += _after(False, False, "a") + _fold(7) + ["done"]
            for x in (1, 2, 3, 4, 5):
                it += _fold(x)
            return it + [A.exit_(), "out", A.mov64_imm(0, 2), A.exit_()]
        it = _prologue(20 if k == "mapptr" else 16)
        it += _store_bytes(10, -40, PAT)
        it += [A.ld_imm64(5, PREFILL), A.stx(8, 10, -64, 8), A.stx(8, 10, -56, 5)]     # an update's value: 24 bytes to r10 - 40
        if k == "mapptr":                                  # the address the packet carries, onto the stack too
            it += [A.ldx(4, 4, 2, 16), A.stx(4, 10, -48, 4)]
            if op == "delete":                             # the key is the vCPU's own, keyc(cpu, 2, K): only h20 holds it
                it += [A.call(A.FN_GET_SMP_PROCESSOR_ID), A.stx(2, 10, -40, 0), A.st(2, 10, -38, 0xC3A2), A.mov64_reg(0, 8)]
        else:
            it += [A.stx(8, 10, -48, 8)]
        if region in ("row", "own"):                       # the lane's pc72 row: the translation cache
            it += _const_key(0) + [A.ld_map_fd(1, "pc72"), A.call(A.FN_MAP_LOOKUP_ELEM), A.jmp("jeq", 0, 0, "out"),
                                   A.mov64_reg(9, 0), A.mov64_reg(0, 8)]
            if region == "row":                            # index 0 at its start, PAT's key bytes from 24
                it += [A.st(4, 9, 0, 0)] + _store_bytes(9, 24, PAT[:20])
            else:                                          # nine different words from the packet's value
                it += [A.mov64_reg(4, 8)]
                for w in range(9):
                    it += [A.stx(8, 9, 8 * w, 4), A.alu64("mul", 4, FOLD_K), A.alu64("add", 4, 5, reg=True)]
        # base + delta in a scratch register
        if k == "mapptr":
            it += [A.ld_map_fd(9, "arr")]
        elif k in ("idx", "budget"):
            it += [A.mov64_imm(9, 0)]
        elif k == "adjtail" or region == "xdp":
            it += [A.mov64_reg(9, 6)]
        elif region == "stack":
            it += [A.mov64_reg(9, 10)]
        elif region == "packet":
            it += [A.mov64_reg(9, 2)]
        it += [A.alu64("add", 9, 7, reg=True)]
        # the arguments
        stack_key = [A.mov64_reg(2, 10), A.alu64("add", 2, -40)]
        value = [A.mov64_reg(3, 10), A.alu64("add", 3, -64)]
        if k == "mapptr" and op in ("lookup", "delete"):
            it += [A.mov64_reg(1, 9)] + stack_key
        elif k == "mapptr":
            it += [A.mov64_reg(1, 6), A.mov64_reg(2, 9), A.mov64_imm(3, 1)]
        elif k == "key":
            it += [A.mov64_reg(2, 9)] + (value if op == "update" else [])
        elif k == "val":
            it += _const_key(2 if mp == "pc72" else 0) + [A.mov64_reg(3, 9)]
        elif k == "idx" and op == "tail":
            it += [A.mov64_reg(1, 6), A.mov64_reg(3, 9)]
        elif k == "idx":
            it += [A.stx(4, 10, -4, 9), A.mov64_reg(2, 10), A.alu64("add", 2, -4)] + (value if op == "update" else [])
        elif k == "adjtail":
            it += [A.mov64_reg(1, 9), A.mov64_imm(2, -4)]
        it += [A.mov64_reg(4, 8)]
        # the map as an LD_IMM64 in the call's own block: the inline forms are generated
        if k in ("key", "val") or (k == "idx" and op != "tail"):
            it += [A.ld_map_fd(1, mp)]
        elif k == "idx":
            it += [A.ld_map_fd(2, "progs")]
        it += ["call", A.call(fn)]
        it += _after(op == "lookup", noaddr, "a")
        for x in (1, 2, 3, 4, 5):
            it += _fold(x)
        # what the call may have changed
        if op == "update" and mp in ("pc24", "pc72"):
            it += _readback(mp, _const_key(0), 3 if mp == "pc24" else 9, "b")
        elif op == "update" and mp == "arrv":              # the entry the lane's index names (the key is still at r10 - 4)
            it += _readback(mp, [A.mov64_reg(2, 10), A.alu64("add", 2, -4)], 0, "b")
        elif k == "mapptr" and op == "delete":             # is the vCPU's key still in the map that held it?
            it += _readback("h20", [A.mov64_reg(2, 10), A.alu64("add", 2, -40)], 0, "b", noaddr=True)
        elif self.mutates_hash:                            # the key the form aims at: K bytes at data + 20
            it += _readback(mp, [A.ldx(4, 2, 6, 0), A.alu64("add", 2, 20)], 0, "b", noaddr=True)
        it += [A.mov64_reg(8, 0), A.call(A.FN_GET_SMP_PROCESSOR_ID)] + _after(False, False, "c")
        return it + [A.exit_(), "out", A.mov64_imm(0, 2), A.exit_()]

    @functools.cached_property
    def asm(self):
        return A.assemble([x for x in self.items if x != "call"])

    @property
    def raw(self):
        return self.asm[0]

    @property
    def relocs(self):
        return self.asm[1]

    @functools.cached_property
    def call_pc(self) -> int:
        """The slot of the lane-varying call."""
        pc = 0
        for x in self.items:
            if x == "call":
                return pc
            if not isinstance(x, str):
                pc += x.slots
        raise AssertionError


def _forms() -> List[Form]:
    fs = [Form("mapptr", "lookup"), Form("mapptr", "tail")]
    fs += [Form("key", "lookup", r, m) for m, rs in (("arr", ("stack", "packet", "xdp", "row")), ("pc24", ("stack", "packet")),
                                                     ("h20", ("stack", "packet", "xdp", "row")), ("h40", ("stack", "packet")),
                                                     ("ph", ("packet",))) for r in rs]
    fs += [Form("key", "update", "stack", "pc72"), Form("key", "update", "packet", "pc72")]
    fs += [Form("val", "update", r, "pc24") for r in ("stack", "packet", "xdp")]
    fs += [Form("val", "update", "own", "pc72"), Form("val", "update", "stack", "pc72")]
    fs += [Form("idx", "lookup", map="arr"), Form("idx", "lookup", map="pc72"), Form("idx", "update", map="pc72"),
           Form("idx", "tail", map="progs"), Form("budget", "tail"), Form("adjtail", "adjust")]
    # the forms that mutate a shared hash map come last, in a VM of their own: the slots their inserts take
    # depend on the order of the vCPUs, and no other form's fold may see them
    fs += [Form("key", "update", "packet", "h20"), Form("key", "delete", "packet", "h20"), Form("key", "delete", "packet", "ph"),
           Form("key", "update", "packet", "ph"), Form("mapptr", "delete"), Form("idx", "update", map="arrv")]
    return fs


@functools.lru_cache(maxsize=None)
def forms() -> Tuple[Form, ...]:
    return tuple(_forms())


CHUNK = 4      # programs per VM next to the three targets: hipRTC time grows steeply with the program count


@functools.lru_cache(maxsize=None)
def chunks():
    """[(first form index, forms)]."""
    fs = forms()
    return [(a, list(fs[a:a + CHUNK])) for a in range(0, len(fs), CHUNK)]


def chunk_of(index: int):
    return next(c for c in chunks() if c[0] <= index < c[0] + len(c[1]))


def one_per_group() -> List[int]:
    """One form per group (six) for the one-program kernels."""
    want = ("mapptr_lookup", "key_row_h20_lookup", "val_own_pc72_update", "idx_progs_tail", "budget_tail", "adjtail_adjust")
    names = [f.name for f in forms()]
    return [names.index(w) for w in want]


TARGETS = tuple(A.assemble(_fold(3)[:1] + [A.alu64("add", 0, c), A.exit_()])[0] for c in T_CONST) + (b"",)


def _init_bytes(tag: int, n: int) -> bytes:
    return bytes(0x30 + ((tag * 37 + 11 * k) % 0x60) for k in range(n))


def keyc(cpu: int, g: int, K: int) -> bytes:
    """The key a hash-mutating form aims at: the vCPU and a generation, then PAT's bytes."""
    return (cpu.to_bytes(2, "little") + bytes([0xA0 + g, 0xC3]) + PAT[4:])[:K]


def _layout(fs) -> Space:
    return Space(V_CPUS, list(MAPS), len(fs) + N_TARGETS)


@functools.lru_cache(maxsize=None)
def _scenario(fs: Tuple[Form, ...]):
    from harness import Scenario

    sp = _layout(fs)
    a32 = lambda a: a.to_bytes(4, "little")          # noqa: E731
    k32 = a32
    obj = lambda n: sp.maps[n]["obj"].addr           # noqa: E731
    t0 = len(fs)
    init = []
    # the plain array: double pointers to a hash map and to the prog array, an unresolved address, a values backing
    words = (obj("h20"), obj("progs"), 5, sp.maps["pc72"]["values"][0].addr)
    for k in range(6):
        init.append(("arr", k32(k), (a32(words[k]) if k < 4 else b"") + _init_bytes(k, 8 if k < 4 else 12), 0))
    for c in (0, 1, 2, 3, V_CPUS - 2, V_CPUS - 1):          # rows another vCPU's lane reads through a sub-array object
        init.append(("pc24", k32(0), _init_bytes(20 + c, 24), c))
        init.append(("pc72", k32(0), _init_bytes(40 + c, 12), c))
    for n in ("h20", "h40"):
        K, S = SPEC[n]["key_size"], SPEC[n]["value_size"]
        init += [(n, PAT[:K], _init_bytes(60 + K, S), 0), (n, bytes(K), _init_bytes(61 + K, S), 0)]
    for c in (0, 1, 2, 3):
        init.append(("ph", PAT[:8], _init_bytes(70 + c, 12), c))
    if any(f.mutates_hash for f in fs):                     # the keys those forms find: one per vCPU
        for c in range(V_CPUS):
            init.append(("h20", keyc(c, 0, 20), _init_bytes(80 + c, 12), 0))
            init.append(("h20", keyc(c, 2, 20), _init_bytes(81 + c, 12), 0))     # the map-pointer delete's key: in h20 alone
            init.append(("ph", keyc(c, 0, 8), _init_bytes(90 + c, 12), c))
    # the prog array: a program, a second one, the empty one, 0, the first one's inclusive end, the byte past the last
    # program (the process's stack), a map object, an unresolved address, the budget form itself, the second program
    slots = [sp.prog_addr[t0], sp.prog_addr[t0 + 1], sp.prog_addr[t0 + 2], 0, sp.prog_addr[t0] + 8, sp.prog_addr[t0 + 2] + 9,
             obj("arr"), 5, 0, sp.prog_addr[t0 + 1]]
    for k, f in enumerate(fs):
        if f.kind == "budget":
            slots[SELF_SLOT] = sp.prog_addr[k]
    assert sp.prog_addr[t0 + 2] + 9 == sp.static_next
    init += [("progs", k32(k), a32(a), 0) for k, a in enumerate(slots) if a]
    progs = [(f"p{k}", f.raw, f.relocs) for k, f in enumerate(fs)] + [(f"t{k}", raw, []) for k, raw in enumerate(TARGETS)]
    return Scenario(vcpus=V_CPUS, maps=[dict(m) for m in MAPS], progs=progs, map_init=init, max_tail_calls=MAX_TAIL)


def scenario(fs):
    return _scenario(tuple(fs))


def space_of(fs) -> Space:
    sc = scenario(fs)
    sp = _layout(fs)
    for name, key, val, cpu in sc.map_init:
        assert sp.update(sp.maps[name], -1, bytes(key), bytes(val), cpu) == 0
    return sp


def decoded(fs, sp):
    return [MM.decode(raw, rel, sp) for _, raw, rel in scenario(fs).progs]


# ---------------------------------------------------------------------------------------------
# packets
# ---------------------------------------------------------------------------------------------
def _around(a: int, size: int):
    return [a - 1, a, a + 1, a + size, a + size + 1]


def _lay(sp: Space, H: int, L: int, T: int):
    St = sp.static_next
    P = St + STACK_SIZE + 1
    return dict(St=St, P=P, M=H + L + T, X=P + H + L + T + 1, H=H, L=L, T=T)


def _split(v: int):
    """(d, hi) of pack() for a 64-bit register value v: v = (s64)d + (hi << 32)."""
    v &= M64
    d = v & M32
    d -= (d >> 31) << 32
    return d, ((v - d) >> 32) & M32


def _region(f: Form, lay):
    """(base offset inside the entry, backing length B) of a key / val form's region."""
    if f.region == "stack":
        return FRAME, STACK_SIZE
    if f.region == "packet":
        return lay["H"], lay["M"]
    if f.region == "xdp":
        return 0, XDP_MD_SIZE
    return 0, 72                                           # the lane's pc72 row


def _good(f: Form, lay):
    """Offsets (inside the entry) at which the form's pointer finds what its generator put there."""
    n = f.size
    if f.region == "stack":
        return [FRAME - 40, FRAME - 64] if f.kind == "val" else [FRAME - 40]
    if f.region == "packet":
        return [lay["H"] + 20]
    if f.region == "xdp":
        return [12, 16, 20] if n == 4 else [0]
    if f.region == "row":
        return [0, 24] if n == 4 else [24]
    return [24 + d for d in range(-11, 12)]                # own: dest +- 1 .. +- (S - 1), both directions


def mapptr_spots(sp: Space, lay, cpu: int):
    """(maps, double pointers) a form-1 pointer may name: object addresses, and addresses of words
    that hold one."""
    objs = [sp.maps[m["name"]]["obj"].addr for m in MAPS]
    dbl = [sp.maps["arr"]["values"][0].addr, sp.maps["arr"]["values"][0].addr + 12, lay["St"] + FRAME - 48, lay["P"] + lay["H"] + 16]
    return objs, dbl


def edges(f: Form, sp: Space, lay, cpu: int) -> List[Tuple[int, int]]:
    """The edge list of form f for one packet: (d, hi) pairs.  Its length does not depend on the
    packet."""
    k = f.kind
    if k == "mapptr":
        base = sp.maps["arr"]["obj"].addr
        t = []
        for m in MAPS:
            t += _around(sp.maps[m["name"]]["obj"].addr, 8)
        for name in ("pc24", "pc72"):                      # sub-array objects: [A, A + 8], the first value byte at A + 9
            for c in (0, cpu, (cpu + 1) % V_CPUS, V_CPUS - 1):
                t += _around(sp.maps[name]["values"][c].addr - 9, 8)
        av = sp.maps["arr"]["values"][0].addr
        t += _around(av, 72) + [av + 12, av + 24, av + 36, av + 68, av + 69]
        r10 = lay["St"] + FRAME
        t += [lay["St"] - 1, lay["St"], r10 - 49, r10 - 48, r10 - 47, lay["St"] + STACK_SIZE - 4, lay["St"] + STACK_SIZE - 3,
              lay["St"] + STACK_SIZE]
        d = lay["P"] + lay["H"]
        t += [lay["P"] - 1, d + 15, d + 16, d + 17, lay["P"] + lay["M"] - 4, lay["P"] + lay["M"] - 3, lay["P"] + lay["M"]]
        t += _around(lay["X"], XDP_MD_SIZE) + _around(sp.prog_addr[-N_TARGETS], 8) + [0, 0xFFFF]
        return [_split(x - base) for x in t]
    if k in ("key", "val"):
        n = f.size
        base, B = _region(f, lay)
        offs = [-1, 0, 1, B - n, B - n + 1, B - 1, B, B + 1] + _good(f, lay)
        if f.region == "packet":
            offs += [lay["H"] - 1, lay["H"] + lay["L"] - n, lay["H"] + lay["L"]]
        return [_split(o - base) for o in offs]
    if k == "idx":
        E = SPEC[f.map]["max_entries"]
        vals = [0, E - 1, E, E + 1, 1 << 31, (1 << 32) - 1]
        if f.map == "arrv":                                # in range only the vCPU's own four entries: 0 is vCPU 0's, E - 1 the last one's
            vals = [4 * cpu + (0 if cpu == 0 else 1), 4 * cpu + (3 if cpu == V_CPUS - 1 else 2), E, E + 1, 1 << 31, (1 << 32) - 1,
                    4 * cpu, 4 * cpu + 3]
        if f.op == "tail":                                 # every slot; the helper uses uint32(R3)
            vals += list(range(1, E - 1)) + [(1 << 32) + 1, (1 << 32) + E, (5 << 32) + 9, (1 << 63) + 4]
        return [_split(v) for v in vals]
    if k == "budget":
        return [_split(v) for v in (0, 1, 2, 32, 33, 34, 35, 40)]
    X, P, M, St = lay["X"], lay["P"], lay["M"], lay["St"]   # adjtail: base = xdp_md
    t = _around(X, XDP_MD_SIZE) + [P - 1, P, P + 1, P + M - 1, P + M, St + FRAME, St + STACK_SIZE, sp.maps["arr"]["obj"].addr,
                                   sp.maps["arr"]["values"][0].addr, sp.maps["h20"]["obj"].addr, sp.prog_addr[0], 0]
    return [_split(x - X) for x in t]


def _random(f: Form, sp: Space, lay, cpu: int, rng) -> Tuple[int, int]:
    k = f.kind
    hi = rng.randint(1, M32) if rng.random() < 0.25 else 0
    if k == "mapptr":
        base = sp.maps["arr"]["obj"].addr
        objs, dbl = mapptr_spots(sp, lay, cpu)
        u = rng.random()
        progs = sp.maps["progs"]["obj"].addr
        if f.op == "tail" and u < 0.5:                     # names the prog array
            t = rng.choice([progs + rng.randint(0, 8), dbl[1], dbl[2], dbl[3]])
        elif f.op == "delete" and u < 0.5:                 # names a hash map (arrays have no Delete)
            t = rng.choice([sp.maps[n]["obj"].addr + rng.randint(0, 8) for n in ("h20", "h20", "h40", "ph")] + [dbl[0], dbl[2], dbl[3]])
        elif u < 0.7:
            c = rng.randrange(V_CPUS)
            pool = objs + [sp.maps[n]["values"][c].addr - 9 for n in ("pc24", "pc72")] * 2
            t = rng.choice(pool) + rng.randint(0, 8) if rng.random() < 0.75 else rng.choice(dbl)
        else:
            t = rng.randint(base - 16, lay["X"] + 40)
        d, _ = _split(t - base)
        return d, hi
    if k in ("key", "val"):
        base, B = _region(f, lay)
        n = f.size
        if rng.random() < 0.45:
            o = rng.choice(_good(f, lay) + [0, B - n])
        else:
            lo, hi_ = {"stack": (-64, 64), "packet": (-16, 40), "xdp": (-8, 8), "row": (-10, 9), "own": (-10, 9)}[f.region]
            if f.mutates_hash:                             # into xdp_md as far as its data_end: one per vCPU (_lens);
                lo, hi_ = -7, 5                            # not into the stack's last bytes: zero for every vCPU
            o = rng.randint(lo, B + hi_)
        return o - base, hi
    if k == "idx":
        E = SPEC[f.map]["max_entries"]
        v = rng.randint(0, E + 2) if rng.random() < 0.8 else rng.getrandbits(32)
        if f.map == "arrv":
            v = 4 * cpu + rng.randint(0, 3) if rng.random() < 0.7 else E + rng.getrandbits(32) % ((1 << 32) - E)
        return _split(v)[0], hi
    if k == "budget":
        return rng.randint(0, 40), hi
    X, P, M = lay["X"], lay["P"], lay["M"]
    u = rng.random()
    t = P + rng.randint(-2, M + 2) if u < 0.6 else X + rng.randint(-4, 30) if u < 0.8 else rng.randint(0x10000 - 16, X + 40)
    return _split(t - X)[0], hi


def _value(rng) -> int:
    return int.from_bytes(bytes(rng.randint(1, 0x5F) for _ in range(8)), "little")


def _lens(f: Form, rng, k: int):
    """(H, L, T) of packet k."""
    H = rng.randint(0, 23) if f.rooms else 0
    T = rng.randint(0, 16) if f.rooms else 0
    if f.kind == "adjtail":                                # half of them exactly 20 bytes of packet memory
        return 0, 20 if k % 4 < 2 else rng.choice((16, 19, 21, 24, 64)), 0
    if f.mutates_hash:                                     # a length per vCPU: a key read from xdp_md is that vCPU's alone
        return 0, 64 + k % V_CPUS, 0
    if f.region == "packet" or f.kind == "mapptr":
        lo = 64
        L = rng.choice((lo, lo + 1, 100, 128, 590, 1514)) if rng.random() < 0.5 else rng.randint(lo, 1514)
        return H, L, T
    return 0, 24, 0


def make_packet(f: Form, sp: Space, k: int, cpu: int, H: int, L: int, T: int, rng, edge: int = -1) -> Tuple[bytes, int, int]:
    """Packet k's bytes (L of them), its 64-bit delta and its edge index."""
    lay = _lay(sp, H, L, T)
    if edge >= 0:
        d, hi = edges(f, sp, lay, cpu)[edge]
    else:
        d, hi = _random(f, sp, lay, cpu, rng)
    if f.mutates_hash and f.kind == "key":                 # the vCPU in every key window that covers the packet's first bytes
        hi = (cpu + 1) | (rng.getrandbits(15) << 16)       # (the helper takes uint32 of the pointer: any bits 32..63 do)
    body = bytearray(MM.pack(d, hi, _value(rng)))
    if f.mutates_hash and f.kind == "key":                 # random bytes: no two packets share a key window
        body += bytes(rng.getrandbits(8) for _ in range(L - 16))
        K = f.size
        body[20:20 + K] = keyc(cpu, (k // V_CPUS) % 2, K)
    else:
        body += bytes(0xE0 + rng.randrange(0x1F) for _ in range(L - 16))
        if f.kind == "mapptr":                             # a map's address: the prog array's three times of four for a tail call
            objs, _ = mapptr_spots(sp, lay, cpu)
            a = sp.maps["progs"]["obj"].addr if f.op == "tail" and k % 8 < 6 else objs[(k // 2) % len(objs)]
            if f.op == "delete" and k % 8 < 6:
                a = sp.maps[("h20", "ph", "h20", "h40")[(k // 8) % 4]]["obj"].addr
            body[16:20] = a.to_bytes(4, "little")
        elif f.region == "packet":
            n = f.size
            if f.kind == "val":
                good = bytes(rng.randint(1, 0x5F) for _ in range(n))
            elif n == 4:
                good = (k % (SPEC[f.map]["max_entries"] + 2)).to_bytes(4, "little")
            else:
                good = PAT[:n]
            body[20:20 + n] = good
            body[L - n:L] = good
    assert len(body) == L
    return bytes(body), (d + (hi << 32)) & M64, edge


@functools.lru_cache(maxsize=None)
def batch_for(fs: Tuple[Form, ...], j: int):
    """The batch of fs[j] in the VM of fs (the stack's address, and so every form-1 and form-6
    delta, depends on how many programs the VM holds): dict(buf, off, lens, cpu, headroom,
    tailroom, delta, edge).  Even packets walk the form's edge list cyclically, odd packets draw from
    the form's neighbourhood; a quarter of the odd packets add random bits 32..63.  Nobody writes the
    arrays."""
    f = fs[j]
    index = forms().index(f)
    sp = _layout(fs)
    rng = random.Random(SEED * 131 + index)
    n = N_PACKETS
    dims = [_lens(f, rng, k) for k in range(n)]
    slot = [max(64, (H + L + T + 63) // 64 * 64) for H, L, T in dims]
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(slot)[:-1]
    buf = np.random.default_rng(SEED + index).integers(0, 256, int(sum(slot)), dtype=np.uint8)   # dirty rooms
    n_edges = len(edges(f, sp, _lay(sp, 0, 64, 0), 0))
    delta, edge = [], []
    for k in range(n):
        H, L, T = dims[k]
        pkt, d, e = make_packet(f, sp, k, k % V_CPUS, H, L, T, rng, (k // 2) % n_edges if k % 2 == 0 else -1)
        o = int(off[k]) + H
        buf[o:o + L] = np.frombuffer(pkt, np.uint8)
        delta.append(d)
        edge.append(e)
    out = dict(buf=buf, off=off, lens=np.array([d[1] for d in dims], np.uint32), cpu=(np.arange(n) % V_CPUS).astype(np.int32),
               headroom=np.array([d[0] for d in dims], np.uint32) if f.rooms else 0,
               tailroom=np.array([d[2] for d in dims], np.uint32) if f.rooms else 0,
               delta=np.array(delta, np.uint64), edge=np.array(edge, np.int32))
    for x in out.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return out


def runs(fs):
    fs = tuple(fs)
    out = []
    for j in range(len(fs)):
        b = batch_for(fs, j)
        out.append(dict(entry=j, buf=b["buf"], off=b["off"], lens=b["lens"], cpu=b["cpu"], headroom=b["headroom"],
                        tailroom=b["tailroom"]))
    return out


def model_sequence(fs, skip_call: bool = False, log: bool = False):
    """The model's run of a VM's sequence (one batch per form, on one address space): per form a dict
    of status / r0 / steps / err_pc / prog arrays and the final packet buffer; then the final map
    bytes {name: [bytes per cpu]} and the hash maps' contents {name: {key: [value per cpu]}}.
    skip_call: out[j]["skip_r0"] holds, for every packet of an update form, R0 of a run with the
    lane-varying call left out, from the state the real run left for it.  log: out[j]["log"] is the
    form's shared-map touch log.  out[j]["outcome"]: what the lane-varying call did (run_process);
    out[j]["map"]: the map it named; out[j]["fill"]: the fullest any hash map got, as a share of
    its capacity."""
    fs = tuple(fs)
    sp = space_of(fs)
    progs = decoded(fs, sp)
    outs = []
    for j, f in enumerate(fs):
        b = batch_for(fs, j)
        n = len(b["lens"])
        st, r0, steps, epc, prog = (np.zeros(n, np.int64), np.zeros(n, np.uint64), np.zeros(n, np.int64), np.zeros(n, np.int64),
                                    np.zeros(n, np.int64))
        buf = b["buf"].copy()
        skip = np.zeros(n, np.uint64)
        outcome, named, fill = [], [], 0.0
        sp.log = [] if log and f.mutating else None
        for k in range(n):
            H, T = MM._rooms(b, k)
            o, L, cpu = int(b["off"][k]), int(b["lens"][k]), int(b["cpu"][k])
            pkt = bytes(buf[o + H:o + H + L])
            if skip_call and f.op == "update" and not f.mutates_hash:
                rows = {nm: bytes(sp.maps[nm]["values"][cpu].mem) for nm in ("pc24", "pc72")}
                skip[k] = run_process(sp, progs, j, pkt, H, T, cpu, skip_pc=f.call_pc)[1]
                for nm, v in rows.items():
                    sp.maps[nm]["values"][cpu].mem[:] = v
            sp.last_map = None
            s = run_process(sp, progs, j, pkt, H, T, cpu, call_pc=f.call_pc)
            outcome.append(s[6])
            named.append(sp.last_map if f.kind == "mapptr" else f.map)
            if f.mutates_hash:
                fill = max([fill] + [len(sp.maps[m["name"]]["slots"]) / m["max_entries"] for m in MAPS if m["type"] in HASHES])
            st[k], r0[k], steps[k], epc[k], prog[k] = s[0], s[1], s[2], s[3], s[5]
            buf[o:o + H + L + T] = np.frombuffer(s[4], np.uint8)
        d = dict(status=st, r0=r0, steps=steps, err_pc=epc, pkt=buf, prog=prog)
        for x in d.values():
            x.setflags(write=False)
        d["outcome"], d["map"], d["fill"] = outcome, named, fill
        if skip_call:
            d["skip_r0"] = skip
        if sp.log is not None:
            d["log"], sp.log = sp.log, None
        outs.append(d)
    maps = {m["name"]: sp.map_values(m["name"]) for m in MAPS}
    hashes = {m["name"]: sp.hash_contents(m["name"]) for m in MAPS if m["type"] in HASHES}
    return outs, maps, hashes


@functools.lru_cache(maxsize=None)
def expected(c: int):
    """The model's run of chunk c (computed once; read-only)."""
    return model_sequence(chunks()[c][1])


def assert_model(fs, j: int, want, got, tag: str):
    """got: a result dict of the batch of fs[j] against the model's `want`."""
    f = fs[j]
    b = batch_for(tuple(fs), j)
    for key in ("status", "r0", "steps", "err_pc"):
        g = np.asarray(got[key]).astype(np.uint64 if key == "r0" else np.int64)
        bad = np.nonzero(g != want[key])[0]
        if len(bad):
            k = int(bad[0])
            raise AssertionError(f"{tag} {f.name} ({f.ref}): {key} differs for {len(bad)} packets {bad[:8].tolist()}, first packet "
                                 f"{k} delta={int(b['delta'][k]):#x} edge={int(b['edge'][k])} len={int(b['lens'][k])} cpu={k % V_CPUS}: "
                                 f"got {int(g[k]):#x} model {int(want[key][k]):#x} (model status {int(want['status'][k])})")
    g = np.asarray(got["pkt"])
    bad = np.nonzero(g[:len(want["pkt"])] != want["pkt"][:len(g)])[0]
    if len(bad):
        k = int(np.searchsorted(b["off"], bad[0], side="right")) - 1
        raise AssertionError(f"{tag} {f.name}: packet memory differs at byte {int(bad[0])} (packet {k}, delta={int(b['delta'][k]):#x})")


def assert_model_maps(fs, want_maps, want_hashes, got_maps, got_hashes, tag: str):
    """Exact to the byte and the slot; the hash maps of a VM whose forms insert into one from many
    vCPUs at once compare by key."""
    by_key = any(f.mutates_hash for f in fs)
    for name, vals in want_maps.items():
        if SPEC[name]["type"] in HASHES:
            wh, gh = want_hashes[name], got_hashes[name]
            assert sorted(wh) == sorted(gh), f"{tag}: hash map {name}: key sets differ ({len(wh)} vs {len(gh)} keys)"
            for key in wh:
                assert [bytes(v) for v in gh[key]] == wh[key], f"{tag}: hash map {name} key {key.hex()}: values differ"
            if by_key:
                continue
        for c, v in enumerate(vals):
            assert bytes(got_maps[name][c]) == v, f"{tag}: map {name} cpu {c} differs from the model"


# Process.Run: the edge list first, then the form's random draws, 32 in all
def proc_cases(fs, j: int):
    """[(packet bytes, cpu)] of 32 single processes for fs[j]: no rooms, four vCPUs so that rows and
    hash entries carry over from process to process."""
    fs = tuple(fs)
    f = fs[j]
    sp = _layout(fs)
    rng = random.Random(SEED + 7 * forms().index(f))
    n_edges = len(edges(f, sp, _lay(sp, 0, 64, 0), 0))
    out = []
    for n in range(32):
        _, L, _ = _lens(f, rng, n)
        pkt, _, _ = make_packet(f, sp, n, n % 4, 0, L, 0, rng, n if n < n_edges else -1)
        out.append((pkt, n % 4))
    return out
