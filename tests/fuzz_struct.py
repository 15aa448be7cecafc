"""Structured eBPF program generator: programs that finish, built at the JIT analyses' preconditions.

`fuzz.py` draws slots at random, so most of its programs die on a bad slot before an optimised
slot runs.  This generator builds programs that are well formed by construction -- every register
has one kind between blocks (r6 the context, r2 / r3 the packet pointers, r7-r9 scalars, r10 the
stack; inside a block a scratch register is a scalar, a packet pointer behind its bounds check, a
stack pointer or a map value behind its null check) and a block only emits slots that are legal
for those kinds -- so nearly every packet reaches EXIT, and what it returns is a fold of
everything the program computed:

* r7 / r8 / r9 are accumulators.  Every loaded packet byte, read-back stack word, readable counter
  and helper result is folded into one of them (xor / add / rotate), and EXIT returns a fold of the
  three, so a wrong value anywhere shows in R0.
* Branches test packet bytes (drawn from a small alphabet by `make_batch`), the packet length and
  get_smp_processor_id, so the lanes of one wave take different paths.
* The blocks sit at the preconditions of jit.cpp's analyses (key forwarding, the deferred key
  store, early loads and windows, fused increments, the lane value cache, spread / owned kernels,
  deferral, inline hash lookups and tail calls).  A *focused* case is one qualifying block in a
  small program; its *neighbours* differ from it in one place that must flip an analysis (or must
  not).  `Case.expect` records what the generator intends: {feature: True (must fire) | False
  (must be refused)}; tests/test_fuzz_struct_cpu.py checks it against the generated source.

`generate(seed)` is deterministic (numpy.random.default_rng only) and calls neither the oracle nor
the engine.  `N_SEEDS` seeds make the corpus; `make_batch(case)` draws the case's packet batch.

Shared maps (plain arrays, hash maps' key index) are only written by programs that run on one
vCPU (`Case.vcpus` is then 1): concurrent vCPUs race on them in the reference's pool too, so
such programs would not be comparable packet by packet.  Per-CPU values are written at any V.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from mimic_amd import asm as A

FEATURES = ("fwd", "elide", "early", "window", "inc", "vc", "lvc", "lds_stack", "spread", "own", "defer",
            "hash_inline", "tail_inline")
LENGTHS = (0, 1, 13, 14, 33, 34, 54, 60, 64, 65, 100, 1514)
LENGTH_W = (0.02, 0.02, 0.03, 0.04, 0.04, 0.05, 0.10, 0.10, 0.25, 0.10, 0.15, 0.10)
ALPHABET = (0, 1, 2, 3, 0x11, 0x80, 0xFF)
N_PACKETS = 1000
STEP_BUDGET = 20000
ACC = (7, 8, 9)
PCPU_ROWS = ((8, 8), (8, 24), (8, 32), (8, 40), (8, 64), (8, 128), (8, 136), (4, 4), (4, 32))   # (S, row bytes)


@dataclass
class Case:
    seed: int
    family: str
    vcpus: int
    maps: List[dict]
    progs: List[Tuple[str, bytes, list]]
    prog_array: List[Tuple[str, int, int]]
    map_init: List[Tuple[str, bytes, bytes, int]]
    blocks: List[str]                      # the building blocks used, in order
    neighbour: Optional[str] = None        # the one-place change, for a neighbour case
    base_seed: Optional[int] = None        # the qualifying case it was derived from
    expect: Dict[str, bool] = field(default_factory=dict)
    branch_bytes: List[int] = field(default_factory=list)   # packet offsets the branches test
    shared_write: bool = False

    def scenario(self):
        from harness import Scenario

        return Scenario(vcpus=self.vcpus, maps=self.maps, progs=self.progs, prog_array=self.prog_array,
                        map_init=self.map_init)


class _Set:
    """The maps and shared facts of one program set."""

    def __init__(self, rng):
        self.rng = rng
        self.maps: List[dict] = []
        self.init: List[Tuple[str, bytes, bytes, int]] = []
        self.prog_array: List[Tuple[str, int, int]] = []
        self.blocks: List[str] = []
        self.branch_bytes: List[int] = []
        self.shared_write = False

    def add_map(self, **m):
        m.setdefault("name", f"m{len(self.maps)}")
        self.maps.append(m)
        return m


class _Prog:
    """One program under construction.  Register use: r6 context, r2 / r3 data / data_end (reloaded
    after every helper), r7-r9 accumulators, r0-r5 scratch that is dead between blocks."""

    def __init__(self, st: _Set, name: str, entry: bool = True):
        self.st, self.rng, self.name = st, st.rng, name
        self.items: list = []
        self.nl = 0
        self.tail: list = []        # functions placed after EXIT
        self.live: List[int] = []   # scratch registers holding a scalar the exit fold must read
        self.emit(A.mov64_reg(6, 1), A.ldx(4, 2, 6, 0), A.ldx(4, 3, 6, 4))
        if entry:
            self.emit(A.mov64_imm(7, int(self.rng.integers(1, 1 << 30))), A.mov64_reg(8, 3),
                      A.alu64("sub", 8, 2, reg=True), A.mov64_imm(9, int(self.rng.integers(1, 1 << 30))))
        else:   # a tail-called program continues its caller's accumulators
            self.emit(A.alu64("xor", 7, int(self.rng.integers(1, 1 << 30))))

    def emit(self, *ins):
        self.items += list(ins)

    def label(self, hint="L"):
        self.nl += 1
        return f"{self.name}_{hint}{self.nl}"

    def acc(self, reg: int, tmp: int = 0):
        """Fold a scalar register into an accumulator: xor, add, or rotate-then-xor (through tmp)."""
        k = int(self.rng.integers(0, 3))
        if k == 0:
            self.emit(A.alu64("xor", 7, reg, reg=True))
        elif k == 1:
            self.emit(A.alu64("add", 8, reg, reg=True))
        else:
            r = int(self.rng.integers(1, 63))
            self.emit(A.mov64_reg(tmp, 9), A.alu64("lsh", 9, r), A.alu64("rsh", tmp, 64 - r), A.alu64("or", 9, tmp, reg=True),
                      A.alu64("xor", 9, reg, reg=True))

    def reload(self):
        self.emit(A.ldx(4, 2, 6, 0), A.ldx(4, 3, 6, 4))

    def length(self, reg: int):
        self.emit(A.mov64_reg(reg, 3), A.alu64("sub", reg, 2, reg=True))

    def finish(self):
        self.emit(A.mov64_reg(0, 7), A.alu64("lsh", 0, 13), A.alu64("xor", 0, 8, reg=True), A.mov64_reg(1, 0),
                  A.alu64("rsh", 1, 7), A.alu64("add", 0, 1, reg=True), A.alu64("add", 0, 9, reg=True))
        for r in self.live:
            self.emit(A.alu64("xor", 0, r, reg=True))
        self.emit(A.exit_())
        self.items += self.tail
        raw, rel = A.assemble(self.items)
        return (self.name, raw, list(rel))


# ---------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------
def blk_cpu_branch(p: _Prog):
    """get_smp_processor_id folded in, and a branch on it."""
    p.st.blocks.append("cpu_branch")
    skip = p.label()
    p.emit(A.call(A.FN_GET_SMP_PROCESSOR_ID), A.mov64_reg(4, 0))
    p.acc(4)
    p.emit(A.jmp("jset", 4, int(p.rng.choice([1, 2, 3])), skip), A.alu64("add", 8, int(p.rng.integers(1, 999))), skip)
    p.reload()


def blk_len_branch(p: _Prog):
    p.st.blocks.append("len_branch")
    skip = p.label()
    p.length(4)
    p.emit(A.jmp(str(p.rng.choice(["jgt", "jlt", "jeq", "jne"])), 4, int(p.rng.choice([13, 14, 34, 60, 64, 100])), skip),
           A.alu64("xor", 7, int(p.rng.integers(1, 1 << 20))), skip)


def blk_pkt_loads(p: _Prog, var: Optional[str] = None, nloads: Optional[int] = None, base_off: Optional[int] = None,
                  beyond: Optional[bool] = None):
    """A bounds check, branches, then packet loads of mixed sizes from one base: some within a
    32-byte span (a window), some beyond it.  var: a neighbour step or a store between the check
    and the loads (store_same / store_alias / store_r10)."""
    rng = p.rng
    p.st.blocks.append("pkt_loads" + (f":{var}" if var else ""))
    skip = p.label("skip")
    b0 = int(rng.integers(0, 9)) if base_off is None else base_off
    n = int(rng.integers(2, 5)) if nloads is None else nloads
    loads = []      # (size, offset)
    for _ in range(n):
        sz = int(rng.choice([1, 2, 4, 8]))
        loads.append((sz, b0 + int(rng.integers(0, 32 - sz + 1))))
    far = rng.random() < 0.5 if beyond is None else beyond
    bare = var in ("single", "span_gt32", "base_rewritten", "jump_mid")   # no tested byte: the loads are all there is
    if var == "single":
        loads = loads[:1]
    elif var == "span_gt32":
        loads = [(4, b0), (2, b0 + 44)]
    elif far and not bare:
        loads.append((int(rng.choice([1, 2, 4])), b0 + int(rng.integers(36, 50))))   # beyond the window
    need = max(max(o + s for s, o in loads), loads[0][1] + 2)
    tb = int(rng.integers(0, min(need, 14)))            # the byte the inner branch tests
    p.emit(A.mov64_reg(4, 2), A.alu64("add", 4, need), A.jmp("jgt", 4, 3, skip, reg=True))
    if var == "store_same":
        p.emit(A.stx(1, 2, loads[0][1], 7))
    elif var == "store_alias":      # mov rX, r2; add rX, k: the bytes overlap the first load's
        k = int(rng.integers(1, 6))
        p.emit(A.mov64_reg(5, 2), A.alu64("add", 5, k), A.stx(2, 5, loads[0][1] - k, 8))
    elif var == "store_r10":        # R10 + 1793 is the packet memory's first byte (stack 2 KiB + 1)
        p.emit(A.stx(1, 10, 1793 + int(rng.integers(0, need)), 9))
    if var == "jump_mid":           # a second way into the middle of the region
        mid = p.label("mid")
        p.emit(A.jmp("jset", 8, 1, mid), A.alu64("xor", 7, 0x5A5A), mid)
    elif not bare:
        p.st.branch_bytes.append(tb)
        p.emit(A.ldx(1, 5, 2, tb), A.jmp("jeq", 5, int(rng.choice(ALPHABET)), skip))
        p.acc(5)
    if var == "base_rewritten":     # the same value, but a new definition of the base after the check
        p.emit(A.ldx(4, 2, 6, 0))
    regs = (1, 4, 5)
    for q, (sz, off) in enumerate(loads):
        p.emit(A.ldx(sz, regs[q % 3], 2, off))
        p.acc(regs[q % 3])
        if var is None and q == 0 and len(loads) > 2 and rng.random() < 0.5:
            p.emit(A.jmp("jset", 1, 0x10, skip))
    p.emit(skip)


def _key_into(p: _Prog, reg: int, mask: int, src: str):
    """reg = a small data-dependent scalar: the vCPU, the packet length or an accumulator, masked."""
    if src == "cpu":
        p.emit(A.call(A.FN_GET_SMP_PROCESSOR_ID), A.mov64_reg(reg, 0))
    elif src == "len":
        p.length(reg)
    else:
        p.emit(A.mov64_reg(reg, 7))
    p.emit(A.alu64("and", reg, mask))


def _pow2_mask(n: int) -> int:
    m = 1
    while m < n + 1:
        m *= 2
    return m - 1


def blk_counter(p: _Prog, m: dict, var: Optional[str] = None, readable: bool = False):
    """A 4-byte key store, map_lookup_elem, a null check and ldx / add / stx on the value: the one
    shape that key forwarding, the deferred key store, the fused increment, the value cache and
    the spread kernels all start from.  var: the neighbour step (see PLAN)."""
    rng = p.rng
    p.st.blocks.append(f"counter[{m['name']}]" + (f":{var}" if var else ""))
    S, E = m["value_size"], m["max_entries"]
    miss = p.label("miss")
    src = str(rng.choice(["cpu", "len", "acc"]))
    _key_into(p, 4, _pow2_mask(E), src)        # sometimes >= E: the lookup misses
    ko = -4 * int(rng.integers(1, 9))
    if var == "st_imm_key":
        p.emit(A.st(4, 10, ko, int(rng.integers(0, E))))
    else:
        p.emit(A.stx(4, 10, ko, 4))
    if var == "key_other_block":
        nb = p.label("nb")
        p.emit(A.ja(nb), nb)
    if var == "addr_stored":
        p.emit(A.mov64_reg(5, 10), A.alu64("add", 5, ko), A.stx(8, 10, -48, 5))
    if var == "two_lookups_one_store":      # two lookups in the block share the one key store
        p.emit(A.mov64_reg(2, 10), A.alu64("add", 2, ko), A.ld_map_fd(1, m["name"]), A.call(A.FN_MAP_LOOKUP_ELEM),
               A.mov64_reg(5, 0))
    p.emit(A.mov64_reg(2, 10), A.alu64("add", 2, ko), A.ld_map_fd(1, m["name"]), A.call(A.FN_MAP_LOOKUP_ELEM))
    if var == "two_lookups_one_store":
        p.emit(A.jmp("jeq", 5, 0, miss))
    if var == "value_addr_folded":
        p.emit(A.mov64_reg(5, 0))
        p.acc(5, tmp=4)
    p.emit(A.jmp("jeq", 0, 0, miss))
    off = 0     # the looked-up value is S bytes
    alu = A.alu32 if (S == 4 and rng.random() < 0.5) else A.alu64
    k = int(rng.integers(1, 1000))
    d = 1
    if var == "cnt_ptr_helper":     # the value pointer as another lookup's key
        p.emit(A.mov64_reg(2, 0), A.ld_map_fd(1, m["name"]), A.call(A.FN_MAP_LOOKUP_ELEM), A.jmp("jeq", 0, 0, miss))
    if var == "cnt_branch":
        p.emit(A.ldx(S, 5, 0, off), A.jmp("jset", 5, 1, miss))
    if var == "cnt_to_stack":
        p.emit(A.ldx(S, 5, 0, off), A.stx(8, 10, -56, 5))
    if var == "add_reg":
        p.emit(A.ldx(S, d, 0, off), A.alu64("add", d, 4, reg=True), A.stx(S, 0, off, d))
    elif var == "alu32_on_8" and S == 8:
        p.emit(A.ldx(S, d, 0, off), A.alu32("add", d, k), A.stx(S, 0, off, d))
    else:
        p.emit(A.ldx(S, d, 0, off), alu("add", d, k), A.stx(S, 0, off, d))
    if var == "reg_read_after" or readable:
        p.acc(d)
    p.emit(miss)
    if var == "second_lookup_later_block":  # ... and one in a later block with no new store
        miss2 = p.label("miss")
        p.emit(A.mov64_reg(2, 10), A.alu64("add", 2, ko), A.ld_map_fd(1, m["name"]), A.call(A.FN_MAP_LOOKUP_ELEM),
               A.jmp("jeq", 0, 0, miss2), A.ldx(S, 3, 0, off), alu("add", 3, 7), A.stx(S, 0, off, 3), miss2)
    if var == "result_after_second":        # the first lookup's pointer (kept in r5: helpers leave
        miss2 = p.label("miss")             # r1-r5 alone) used after a second lookup
        p.emit(A.st(4, 10, ko, 0), A.mov64_reg(2, 10), A.alu64("add", 2, ko), A.ld_map_fd(1, m["name"]),
               A.call(A.FN_MAP_LOOKUP_ELEM), A.jmp("jeq", 0, 0, miss2), A.mov64_reg(5, 0),
               A.stx(4, 10, ko, 4), A.mov64_reg(2, 10), A.alu64("add", 2, ko), A.ld_map_fd(1, m["name"]),
               A.call(A.FN_MAP_LOOKUP_ELEM), A.ldx(S, 3, 5, 0), alu("add", 3, 3), A.stx(S, 5, 0, 3), miss2)
    if var == "readback_r10":
        p.emit(A.ldx(4, 5, 10, ko))
        p.acc(5)
    if var == "readback_copy":
        p.emit(A.mov64_reg(4, 10), A.ldx(4, 5, 4, ko))
        p.acc(5)
    p.reload()


def blk_helper_base(p: _Prog, ro: dict):
    """A load through a helper-returned base: a lookup in a second, read-only array."""
    p.st.blocks.append(f"helper_base[{ro['name']}]")
    miss = p.label("miss")
    _key_into(p, 4, _pow2_mask(ro["max_entries"]), "len")
    p.emit(A.stx(4, 10, -40, 4), A.mov64_reg(2, 10), A.alu64("add", 2, -40), A.ld_map_fd(1, ro["name"]),
           A.call(A.FN_MAP_LOOKUP_ELEM), A.jmp("jeq", 0, 0, miss), A.ldx(8, 5, 0, 0))
    p.acc(5)
    p.emit(miss)
    p.reload()


def blk_hash(p: _Prog, m: dict, var: Optional[str] = None, write: bool = False):
    """A hash-map lookup whose key is built from 4-byte stack stores (the first word of a wider
    key is a forwarding candidate); the value is folded in.  write (one vCPU only): a
    map_update_elem of a missing key and a map_delete_elem of some found ones."""
    rng = p.rng
    K = m["key_size"]
    p.st.blocks.append(f"hash[{m['name']},K={K}]" + (f":{var}" if var else "") + (":write" if write else ""))
    miss, done = p.label("miss"), p.label("done")
    ko = -8 * int(rng.integers(1, 4)) - K
    ko -= ko % 4
    if var == "ldimm_other_block":
        nb = p.label("nb")
        p.emit(A.ld_map_fd(1, m["name"]), A.ja(nb), nb)
    _key_into(p, 4, 15, str(rng.choice(["len", "acc"])))
    for q in range(K // 4):
        if q == 0:
            p.emit(A.stx(4, 10, ko, 4))
        else:
            p.emit(A.st(4, 10, ko + 4 * q, 0x01010101 * q))
    p.emit(A.mov64_reg(2, 10), A.alu64("add", 2, ko))
    if var != "ldimm_other_block":
        p.emit(A.ld_map_fd(1, m["name"]))
    p.emit(A.call(A.FN_MAP_LOOKUP_ELEM), A.jmp("jeq", 0, 0, miss), A.ldx(8, 5, 0, 0))
    p.acc(5)
    if write:
        p.st.shared_write = True
        p.emit(A.jmp("jset", 5, 4, done), A.mov64_reg(2, 10), A.alu64("add", 2, ko), A.ld_map_fd(1, m["name"]),
               A.call(A.FN_MAP_DELETE_ELEM), A.mov64_reg(5, 0))
        p.acc(5)
    p.emit(A.ja(done), miss)
    if write:
        p.emit(A.stx(8, 10, ko - 8, 7), A.mov64_reg(2, 10), A.alu64("add", 2, ko), A.mov64_reg(3, 10), A.alu64("add", 3, ko - 8),
               A.mov64_imm(4, 0), A.ld_map_fd(1, m["name"]), A.call(A.FN_MAP_UPDATE_ELEM), A.mov64_reg(5, 0))
        p.acc(5)
    else:
        p.emit(A.alu64("add", 8, 0x777))
    p.emit(done)
    p.reload()


def hash_key(v: int, K: int) -> bytes:
    return b"".join([(v & 0xF).to_bytes(4, "little")] + [(0x01010101 * q).to_bytes(4, "little") for q in range(1, K // 4)])


def blk_update_cached(p: _Prog, m: dict):
    """map_update_elem on a per-CPU array the lane value cache may hold, then the row read back:
    the cache must be written back before the helper and reloaded after."""
    p.st.blocks.append(f"update_cached[{m['name']}]")
    S, E = m["value_size"], m["max_entries"]
    miss = p.label("miss")
    _key_into(p, 4, _pow2_mask(E), "len")
    p.emit(A.stx(4, 10, -12, 4), A.stx(8, 10, -24, 8), A.mov64_reg(2, 10), A.alu64("add", 2, -12), A.mov64_reg(3, 10),
           A.alu64("add", 3, -24), A.mov64_imm(4, 0), A.ld_map_fd(1, m["name"]), A.call(A.FN_MAP_UPDATE_ELEM), A.mov64_reg(5, 0))
    p.acc(5)
    p.emit(A.mov64_reg(2, 10), A.alu64("add", 2, -12), A.ld_map_fd(1, m["name"]), A.call(A.FN_MAP_LOOKUP_ELEM),
           A.jmp("jeq", 0, 0, miss), A.ldx(S, 5, 0, 0))
    p.acc(5)
    p.emit(miss)
    p.reload()


def blk_stack(p: _Prog, var: Optional[str] = None):
    """Stores and read-backs in and around the LDS window [128, 256) of frame 0 (R10 - 128 is its
    lower edge): unaligned, straddling the edge, through R10 and through a copy of it."""
    rng = p.rng
    p.st.blocks.append("stack" + (f":{var}" if var else ""))
    copy_only = var == "copy_only"
    p.emit(A.mov64_reg(5, 10))
    for k in range(int(rng.integers(2, 5))):
        sz = int(rng.choice([1, 2, 4, 8]))
        o = -int(rng.choice([128, 129, 130, 131, 132, 135, 136, 127, 126, 121, 120, 200, 64, 8, 255]))
        o = max(o, -256)
        o = min(o, -sz)
        base = 5 if (copy_only or (k and rng.random() < 0.4)) else 10    # the first one through R10 itself
        p.emit(A.stx(sz, base, o, int(rng.choice(ACC))))
        sz2 = int(rng.choice([1, 2, 4, 8]))
        o2 = min(max(o + int(rng.integers(-7, 8)), -256), -sz2)
        p.emit(A.ldx(sz2, 4, 5 if (copy_only or rng.random() < 0.5) else 10, o2))
        p.acc(4)


def blk_loop(p: _Prog):
    """A loop bounded by construction: 1..32 iterations, the back jump at the end of the body."""
    rng = p.rng
    p.st.blocks.append("loop")
    top = p.label("top")
    if rng.random() < 0.5:
        p.emit(A.mov64_imm(4, int(rng.integers(1, 33))))
    else:
        p.length(4)
        p.emit(A.alu64("and", 4, 31), A.alu64("add", 4, 1))
    p.emit(A.stx(8, 10, -72, 4), top, A.alu64("add", 8, 4, reg=True), A.alu64("lsh", 7, 1), A.alu64("xor", 7, 8, reg=True))
    if rng.random() < 0.5:
        p.emit(A.ldx(8, 5, 10, -72), A.alu64("add", 5, 3), A.stx(8, 10, -72, 5))
    p.emit(A.alu64("add", 4, -1), A.jmp("jne", 4, 0, top), A.ldx(8, 5, 10, -72))
    p.acc(5)


def blk_tail_call(p: _Prog, pa: dict, var: Optional[str] = None):
    """A tail call whose index comes from a packet byte: it may miss or pick an empty slot."""
    rng = p.rng
    p.st.blocks.append("tail_call" + (f":{var}" if var else ""))
    skip = p.label("skip")
    k = int(rng.integers(0, 14))
    p.st.branch_bytes.append(k)
    if var == "ldimm_other_block":
        p.emit(A.ld_map_fd(5, pa["name"]))
    p.emit(A.mov64_reg(4, 2), A.alu64("add", 4, k + 1), A.jmp("jgt", 4, 3, skip, reg=True), A.ldx(1, 3, 2, k),
           A.alu64("and", 3, 7), A.mov64_reg(1, 6))
    if var == "ldimm_other_block":
        p.emit(A.mov64_reg(2, 5))
    elif var == "via_mov":
        p.emit(A.ld_map_fd(4, pa["name"]), A.mov64_reg(2, 4))
    else:
        p.emit(A.ld_map_fd(2, pa["name"]))
    p.emit(A.call(A.FN_TAIL_CALL))
    p.reload()
    p.emit(A.alu64("add", 8, 0x3131), skip)
    return k


def blk_pkt_store_index(p: _Prog, k: int):
    """Rewrite the tail-call index byte (the entry program, when re-entered, takes another way)."""
    p.st.blocks.append("pkt_store_index")
    skip = p.label("skip")
    p.emit(A.mov64_reg(4, 2), A.alu64("add", 4, k + 1), A.jmp("jgt", 4, 3, skip, reg=True), A.ldx(1, 5, 2, k),
           A.alu64("add", 5, 1), A.stx(1, 2, k, 5), skip)


def blk_call(p: _Prog, m: Optional[dict], depth: int, pad: bool = True):
    """A BPF-to-BPF call, one or two frames deep; the callee uses its frame's stack and a lookup,
    and overwrites r7 (the caller must see its own r7 again: r6-r9 are restored on return).  A call
    lands one slot before its target (the reference's quirk Q12, vm.go:163-169 / inst.go:253), so
    every function starts with a pad slot in front of its label: the callee's first step.  pad=False
    leaves the pads out: every call then lands on the EXIT in front of its target and returns at once
    (legal input too; the `calls_land_on_exit` neighbours keep it in the corpus)."""
    rng = p.rng
    p.st.blocks.append(f"call[depth={depth}]")
    f = p.label("fn")
    p.emit(A.mov64_reg(1, 7), A.mov64_reg(2, 8), A.call_local(f), A.mov64_reg(5, 0))
    p.acc(5)
    p.reload()
    pads = [A.mov64_imm(5, 0)] if pad else []
    body = pads + [f, A.stx(8, 10, -8, 1), A.stx(4, 10, -12, 2), A.ldx(4, 0, 10, -6), A.ldx(2, 3, 10, -12), A.alu64("add", 0, 3, reg=True),
            A.mov64_imm(7, 0x55), A.stx(8, 10, -24, 0)]
    if m is not None:
        miss = p.label("miss")
        S = m["value_size"]
        body += [A.alu64("and", 2, _pow2_mask(m["max_entries"])), A.stx(4, 10, -28, 2), A.mov64_reg(2, 10), A.alu64("add", 2, -28),
                 A.ld_map_fd(1, m["name"]), A.call(A.FN_MAP_LOOKUP_ELEM), A.jmp("jeq", 0, 0, miss), A.ldx(S, 1, 0, 0),
                 A.alu64("add", 1, 1), A.stx(S, 0, 0, 1), miss]
    if depth > 1:
        g = p.label("fn")
        body += [A.ldx(8, 1, 10, -24), A.call_local(g), A.ldx(8, 3, 10, -24), A.alu64("xor", 0, 3, reg=True), A.exit_()] + pads + [
                 g, A.stx(8, 10, -16, 1), A.ldx(4, 0, 10, -14), A.alu64("add", 0, 0x99), A.exit_()]
    else:
        body += [A.ldx(8, 0, 10, -24), A.exit_()]
    p.tail += body


# ---------------------------------------------------------------------------------------------
# sets
# ---------------------------------------------------------------------------------------------
def _pcpu_map(st: _Set, S: int, row: int, name: Optional[str] = None) -> dict:
    return st.add_map(name=name or f"pc{len(st.maps)}", type=6, key_size=4, value_size=S, max_entries=row // S)


def _hash_map(st: _Set, K: int, percpu: bool) -> dict:
    return st.add_map(name=f"h{len(st.maps)}", type=5 if percpu else 1, key_size=K, value_size=8, max_entries=12)


def _init_hash(st: _Set, m: dict, V: int):
    for v in range(0, 16, 2):      # every other key present: hits and misses
        for c in (range(V) if m["type"] == 5 else [0]):
            st.init.append((m["name"], hash_key(v, m["key_size"]), (v * 1000 + 7 * c + 3).to_bytes(8, "little"), c))


def _site_count(progs) -> int:
    """jit.cpp's slow-path site count: every LDX / ST / STX / helper call, twice with loops or
    BPF-to-BPF calls (more than 48: the kernel defers its slow paths)."""
    n, careful = 0, False
    for _, raw, _ in progs:
        i = 0
        while i < len(raw) // 8:
            op, regs = raw[8 * i], raw[8 * i + 1]
            off = int.from_bytes(raw[8 * i + 2:8 * i + 4], "little", signed=True)
            cls = op & 7
            if cls in (A.LDX, A.ST, A.STX):
                n += 1
            if cls == A.JMP and (op & 0xF0) == A.CALL:
                if regs >> 4 == A.PSEUDO_CALL:
                    careful = True
                else:
                    n += 1
            if cls in (A.JMP, A.JMP32) and (op & 0xF0) not in (A.CALL, A.EXIT) and off < 0:
                careful = True
            i += 2 if op == (A.LD | A.IMM | A.DW) else 1
    return n * (2 if careful else 1)


def _counter_case(rng, row_pick, var, extra):
    """Family `counter`: a packet-load block and one counter block on one per-CPU array."""
    st = _Set(rng)
    S, row = row_pick
    m = _pcpu_map(st, S, row, "cnt")
    ro = None
    if var == "helper_base":
        ro = st.add_map(name="ro", type=2, key_size=4, value_size=8, max_entries=4)
        for k in range(4):
            st.init.append(("ro", k.to_bytes(4, "little"), (0x1111 * (k + 1)).to_bytes(8, "little"), 0))
    p = _Prog(st, "p0")
    blk_pkt_loads(p)
    if extra == "cpu":
        blk_cpu_branch(p)
    elif extra == "len":
        blk_len_branch(p)
    if var == "helper_base":
        blk_helper_base(p, ro)
        blk_counter(p, m)
    else:
        blk_counter(p, m, var)
    return st, [p.finish()]


COUNTER_EXPECT = {   # neighbour step -> what it must flip (the rest stays as in the qualifying case)
    None: {},
    "readback_r10": {"elide": False, "lds_stack": True},
    "readback_copy": {"elide": False, "lds_stack": True},
    "addr_stored": {"elide": False, "lds_stack": True},
    "key_other_block": {"fwd": False, "elide": False, "lds_stack": True},
    "st_imm_key": {"elide": False, "lds_stack": True},
    "second_lookup_later_block": {"elide": False, "lds_stack": True},
    "two_lookups_one_store": {},
    "value_addr_folded": {},
    "reg_read_after": {"inc": False, "spread": False, "own": False},
    "add_reg": {"inc": False, "spread": False, "own": False},
    "alu32_on_8": {"inc": False, "spread": False, "own": False},
    "cnt_branch": {"spread": False, "own": False},
    "cnt_to_stack": {"spread": False, "own": False, "lds_stack": True},
    "cnt_ptr_helper": {"spread": False, "own": False, "elide": False, "lds_stack": True},
    "helper_base": {"spread": False, "own": False},
    "result_after_second": {"lds_stack": True},
}


def _counter_expect(row_pick, var):
    S, row = row_pick
    cacheable = row % 8 == 0 and row <= 128
    e = {"fwd": True, "elide": True, "inc": True, "spread": True, "own": True, "lds_stack": False,
         "vc": cacheable and row <= 32, "lvc": cacheable and row > 32, "defer": False}
    if not (var == "alu32_on_8" and S != 8):
        e.update(COUNTER_EXPECT[var])
    if row % 8:                           # the engine spreads rows of whole 8-byte words only
        e["spread"] = e["own"] = False
    if var == "result_after_second" and row % 8 == 0:      # no claim on the spread analysis: parity decides
        e.pop("spread"), e.pop("own")
    return e


def _loads_case(rng, var):
    st = _Set(rng)
    p = _Prog(st, "p0")
    blk_len_branch(p)
    blk_pkt_loads(p, var, nloads=3, base_off=0, beyond=False)
    return st, [p.finish()]


# neighbours that must leave every intended decision as it is in their base ("must still accept")
STILL_ACCEPT = ("two_lookups_one_store", "value_addr_folded", "store_same", "store_alias", "store_r10",
                "calls_land_on_exit")

LOADS_EXPECT = {
    None: {"early": True, "window": True},
    "base_rewritten": {"early": False, "window": False},
    "jump_mid": {"early": False, "window": False},
    "span_gt32": {"early": True, "window": False},
    "single": {"early": True, "window": False},
    "store_same": {"early": True},
    "store_alias": {"early": True},
    "store_r10": {"early": True, "window": True},
}


def _hash_case(rng, K, percpu, var, V):
    st = _Set(rng)
    m = _hash_map(st, K, percpu)
    p = _Prog(st, "p0")
    blk_pkt_loads(p)
    w = bool(rng.random() < 0.6)       # drawn for the neighbour too: the same random stream as its base
    blk_hash(p, m, var, write=(var is None and w))    # a writer runs on one vCPU (generate)
    if var is None:
        blk_stack(p)
    return st, [p.finish()]


def _chain_case(rng, nprogs, var, with_counter):
    """Two to four programs joined by a prog array.  The entry's index comes from a packet byte;
    each later program calls the next by a constant index, and the last one rewrites the index
    byte and calls the entry program again: a chain that re-enters it after a packet store."""
    st = _Set(rng)
    pa = st.add_map(name="pa", type=3, key_size=4, value_size=4, max_entries=int(rng.choice([4, 8])))
    m = _pcpu_map(st, 8, 32, "cnt") if with_counter else None
    slots = [int(x) for x in rng.permutation(4)[:nprogs]]     # the rest (and 4..7 of 8) stay empty
    st.prog_array = [("pa", s, i) for i, s in enumerate(slots)]
    progs = []
    k = None
    for i in range(nprogs):
        p = _Prog(st, f"p{i}", entry=(i == 0))
        if i == 0:
            blk_pkt_loads(p)
            k = blk_tail_call(p, pa, var)
            blk_len_branch(p)
        else:
            if m is not None and rng.random() < 0.7:
                blk_counter(p, m, readable=True)
            else:
                blk_stack(p)
            if i == nprogs - 1:
                blk_pkt_store_index(p, k)
            p.st.blocks.append("tail_call:next")
            p.emit(A.mov64_reg(1, 6))
            if var is None:
                p.emit(A.ld_map_fd(2, pa["name"]))
            else:
                p.emit(A.ld_map_fd(4, pa["name"]), A.mov64_reg(2, 4))
            p.emit(A.mov64_imm(3, slots[(i + 1) % nprogs]), A.call(A.FN_TAIL_CALL))
            p.reload()
        progs.append(p.finish())
    return st, progs


def _general_case(rng, V, kind, big=False, sites_max=None, pad=True, nblocks=None):
    """A random mix of blocks.  kind: plain | loop | call | chain."""
    st = _Set(rng)
    S, row = PCPU_ROWS[int(rng.integers(0, len(PCPU_ROWS)))]
    pc = _pcpu_map(st, S, row)
    hm = _hash_map(st, int(rng.choice([4, 8, 16, 40])), bool(rng.integers(0, 2)))
    sh = st.add_map(name="arr", type=2, key_size=4, value_size=8, max_entries=4)
    for k in range(4):
        st.init.append(("arr", k.to_bytes(4, "little"), (0x0101 * (k + 3)).to_bytes(8, "little"), 0))
    p = _Prog(st, "p0")
    menu = ["loads", "loads_store", "counter", "hash", "stack", "cpu", "len", "update", "ro"]
    if kind == "loop":
        menu += ["loop", "loop"]
    if kind == "call":
        menu += ["call", "call"]
    n = int(rng.integers(5, 9)) * (3 if big else 1)
    must = {"loop": ["loop"], "call": ["call"]}.get(kind, [])
    picks = must + [str(rng.choice(menu)) for _ in range(n - len(must))]
    rng.shuffle(picks)
    for b in picks[:nblocks]:
        before = (list(p.items), list(p.tail), list(st.blocks), st.shared_write, list(st.branch_bytes))
        if b == "loads":
            blk_pkt_loads(p)
        elif b == "loads_store":
            blk_pkt_loads(p, str(rng.choice(["store_same", "store_alias", "store_r10"])))
        elif b == "counter":
            blk_counter(p, pc, readable=bool(rng.integers(0, 2)))
        elif b == "hash":
            blk_hash(p, hm, write=bool(rng.random() < 0.15))
        elif b == "stack":
            blk_stack(p)
        elif b == "cpu":
            blk_cpu_branch(p)
        elif b == "len":
            blk_len_branch(p)
        elif b == "update":
            blk_update_cached(p, pc)
        elif b == "ro":
            blk_helper_base(p, sh)
        elif b == "loop":
            blk_loop(p)
        elif b == "call":
            blk_call(p, pc if rng.random() < 0.6 else None, int(rng.integers(1, 3)), pad)
        if sites_max is not None:
            trial = _Prog.__new__(_Prog)
            trial.__dict__.update(p.__dict__)
            trial.items, trial.tail = list(p.items), list(p.tail)
            if _site_count([trial.finish()]) > sites_max:   # leave this block out
                p.items, p.tail, st.blocks, st.shared_write, st.branch_bytes = before
    return st, [p.finish()]


# ---------------------------------------------------------------------------------------------
# the plan: seed -> (family, parameters).  A neighbour names its base seed and is rebuilt from the
# base's random stream with one step changed.
# ---------------------------------------------------------------------------------------------
def _plan():
    plan = []
    rows = [(8, 8), (8, 24), (8, 32), (4, 32), (8, 40), (8, 64), (8, 128), (8, 40), (8, 136), (4, 4)]
    steps = [s for s in COUNTER_EXPECT if s is not None] + ["key_other_block"] * 3 + ["reg_read_after"]
    si = 0
    for i, rp in enumerate(rows):
        base = len(plan)
        extra = ("cpu", "len", None)[i % 3]
        plan.append(("counter", dict(row=rp, var=None, extra=extra)))
        for _ in range(3 if i == 0 else 2):
            plan.append(("counter", dict(row=rp, var=steps[si % len(steps)], extra=extra, base=base)))
            si += 1
    lsteps = [s for s in LOADS_EXPECT if s is not None] + ["base_rewritten", "jump_mid"]
    for i in range(4):
        base = len(plan)
        plan.append(("loads", dict(var=None)))
        for j in range(-(-len(lsteps) // 4)):
            if 4 * j + i < len(lsteps):
                plan.append(("loads", dict(var=lsteps[4 * j + i], base=base)))
    for i, K in enumerate([4, 8, 16, 40]):
        base = len(plan)
        plan.append(("hash", dict(K=K, percpu=bool(i % 2), var=None)))
        plan.append(("hash", dict(K=K, percpu=bool(i % 2), var="ldimm_other_block", base=base)))
    for i in range(8):
        base = len(plan)
        plan.append(("chain", dict(nprogs=2 + i % 3, var=None, counter=bool(i % 2))))
        if i < 4:
            plan.append(("chain", dict(nprogs=2 + i % 3, var=("ldimm_other_block", "via_mov")[i % 2], counter=bool(i % 2), base=base)))
    for i in range(4):      # stack stores through R10 / only through a copy of it
        base = len(plan)
        plan.append(("stack", dict(var=None)))
        plan.append(("stack", dict(var="copy_only", base=base)))
    for i in range(8):      # large enough to defer; the neighbour stops at 48 sites
        base = len(plan)
        plan.append(("general", dict(kind=("plain", "loop", "call", "plain")[i % 4], big=True)))
        if i < 4:
            plan.append(("general", dict(kind=("plain", "loop", "call", "plain")[i % 4], big=True, sites_max=48, base=base)))
    for i in range(8):
        plan.append(("general", dict(kind=("plain", "loop", "call", "plain")[i % 4], big=False)))
    # every general case with calls once more without the functions' pad slots (appended: the seeds
    # above keep their numbers)
    for base, (fam, prm) in enumerate(list(plan)):
        if fam == "general" and prm["kind"] == "call" and "base" not in prm:
            plan.append(("general", dict(prm, pad=False, base=base)))
    return plan


PLAN = _plan()
N_SEEDS = len(PLAN)


def generate(seed: int) -> Case:
    family, prm = PLAN[seed]
    base = prm.get("base")
    rng = np.random.default_rng(0x5EED0000 + (seed if base is None else base))
    V = int(rng.choice([1, 7, 64]))
    expect: Dict[str, bool] = {}
    var = prm.get("var")
    if family == "counter":
        st, progs = _counter_case(rng, prm["row"], var, prm["extra"])
        expect = _counter_expect(prm["row"], var)
        if V == 1:
            V = int(rng.choice([7, 64]))   # the owned form needs 2..256 packets per vCPU
    elif family == "loads":
        st, progs = _loads_case(rng, var)
        expect = dict(LOADS_EXPECT[var], defer=False)
    elif family == "hash":
        st, progs = _hash_case(rng, prm["K"], prm["percpu"], var, V)
        expect = {"hash_inline": var is None, "defer": False}
    elif family == "chain":
        st, progs = _chain_case(rng, prm["nprogs"], var, prm["counter"])
        expect = {"tail_inline": var is None, "elide": False, "spread": False, "own": False}
    elif family == "stack":
        st = _Set(rng)
        p = _Prog(st, "p0")
        blk_pkt_loads(p)
        blk_stack(p, var)
        progs = [p.finish()]
        expect = {"lds_stack": var is None, "defer": False}
    else:
        st, progs = _general_case(rng, V, prm["kind"], prm.get("big", False), prm.get("sites_max"), prm.get("pad", True),
                                  prm.get("nblocks"))
        if prm.get("big"):
            expect = {"defer": prm.get("sites_max") is None}
        if V == 1 and not st.shared_write:
            V = int(rng.choice([7, 64]))   # one vCPU is for the sets that write shared maps (and the focused cases)
    if st.shared_write:
        V = 1
    for m in st.maps:
        if m["type"] in (1, 5) and not any(i[0] == m["name"] for i in st.init):
            _init_hash(st, m, V)
    maps = [dict(m) for m in st.maps]
    return Case(seed=seed, family=family, vcpus=V, maps=maps, progs=progs, prog_array=st.prog_array, map_init=st.init,
                blocks=st.blocks, neighbour=(var or ("sites_le_48" if prm.get("sites_max") else "calls_land_on_exit")) if base is not None else None, base_seed=base, expect=expect,
                branch_bytes=sorted(set(st.branch_bytes)), shared_write=st.shared_write)


def prefix_case(base: int, nblocks: int, pad: bool = True) -> Case:
    """The general case `base` cut after its first `nblocks` blocks (the same random stream up to
    there), with or without the functions' pad slots: for narrowing a difference down."""
    family, prm = PLAN[base]
    assert family == "general" and "base" not in prm
    PLAN.append((family, dict(prm, pad=pad, nblocks=nblocks, base=base)))
    try:
        c = generate(len(PLAN) - 1)
    finally:
        PLAN.pop()
    c.neighbour = f"first_{nblocks}_blocks" + ("" if pad else ",calls_land_on_exit")
    return c


def site_count(case: Case) -> int:
    return _site_count(case.progs)


def make_batch(case: Case, n: int = N_PACKETS, salt: int = 0, sched: Optional[str] = None, rooms: Optional[bool] = None):
    """The case's packet batch: lengths from LENGTHS, random bytes with the branch-tested bytes
    from ALPHABET, a schedule (explicit / chunked / interleaved) and, for a third of the seeds,
    per-packet headroom / tailroom arrays with dirty room bytes (sched / rooms: given instead of
    drawn).  Returns a dict: buf, off, lens, cpu, sched, headroom, tailroom."""
    rng = np.random.default_rng(0xBA7C0000 + case.seed * 16 + salt)
    lens = rng.choice(LENGTHS, n, p=np.asarray(LENGTH_W) / sum(LENGTH_W)).astype(np.uint32)
    rooms = case.seed % 3 == 1 if rooms is None else rooms
    H = rng.integers(0, 24, n).astype(np.uint32) if rooms else 0
    T = rng.integers(0, 17, n).astype(np.uint32) if rooms else 0
    slot = ((H + lens.astype(np.int64) + T + 63) // 64 * 64).astype(np.int64)
    slot = np.maximum(slot, 64)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(slot)[:-1].astype(np.uint64)
    buf = rng.integers(0, 256, int(slot.sum()), dtype=np.uint8)      # room bytes dirty: the run must zero them
    for i in range(n):
        d0 = int(off[i]) + (int(H[i]) if rooms else 0)
        for b in case.branch_bytes:
            if b < int(lens[i]):
                buf[d0 + b] = ALPHABET[int(rng.integers(0, len(ALPHABET)))]
    drawn = ("explicit", "chunked", "interleaved")[int(rng.integers(0, 3))]
    sched = sched or drawn
    V = case.vcpus
    if sched == "explicit":
        cpu = rng.integers(0, V, n).astype(np.int32)
    elif sched == "chunked":
        cpu = (np.arange(n) // -(-n // V)).astype(np.int32)
    else:
        cpu = (np.arange(n) % V).astype(np.int32)
    return dict(buf=buf, off=off, lens=lens, cpu=cpu, sched=sched, headroom=H, tailroom=T)


# ---------------------------------------------------------------------------------------------
# what the JIT decided for a case, read from the generated source (used by the CPU gates and by
# tools/corpus_quality.py; the generator above never calls these)
# ---------------------------------------------------------------------------------------------
def kernel_args(case: Case):
    """(raws, ctx, vc): jit.kernel_source's arguments for the case's default kernel."""
    from mimic_amd import jit as J

    return [raw for _, raw, _ in case.progs], 0, J.vc_slots([(raw, rel) for _, raw, rel in case.progs], case.maps)


def spread_args(case: Case, own: bool = False):
    from mimic_amd import jit as J

    return J.spread_spec([(raw, rel) for _, raw, rel in case.progs], case.maps, case.vcpus, own=own)


def _inline_lookup_of_a_hash_map(case: Case, src: str) -> bool:
    """An inline lookup site (`hash_lookup_fast` behind the array form) whose map hint comes from an
    LD_IMM64 slot that the relocations give to a hash map: the site names the slot in kp.insns."""
    import re

    kind = {m["name"]: m["type"] for m in case.maps}
    slot_map, base = {}, 0
    for _, raw, rel in case.progs:
        for r in rel:
            slot_map[base + r[0]] = r[1]
        base += len(raw) // 8
    for m in re.finditer(r"mh_ = AUX_MAPHINT\(cget\(kp\.insns, (\d+)u\)\.aux\);(.*?)\n(.*?)\n(.*?)\n", src):
        if "hash_lookup_fast(kp, L" in m.group(0) and kind.get(slot_map.get(int(m.group(1)))) in (1, 5):
            return True
    return False


def source_features(case: Case) -> Dict[str, bool]:
    """Which analyses fired, read the way test_jit_cpu.py and test_spread_cpu.py read a kernel."""
    import re

    from mimic_amd import jit as J

    raws, ctx, vc = kernel_args(case)
    src = J.kernel_source(raws, ctx, vc)
    f = {
        "fwd": re.search(r"uint32_t fwd\d+_\d+_ = 0;", src) is not None,
        "elide": "key store deferred into the lookup's cold path" in src,
        "early": re.search(r"sp\d+_\d+_ = 0;   // packet load of", src) is not None,
        "window": "// window of " in src,
        "inc": ": counter increment of r" in src,
        "vc": re.search(r"(?<!l)vc_open\(", src) is not None,
        "lvc": "lvc_open(" in src,
        "lds_stack": "#define MIMIC_LDS_STACK_Q" in src,
        "defer": "#define MIMIC_COLD_INLINE 0" in src and "L_defer:" in src,
        "hash_inline": _inline_lookup_of_a_hash_map(case, src),
        "tail_inline": "tail_fast(kp, L" in src,
    }
    f["spread"] = J.spread_source(raws, *spread_args(case))[1]
    f["own"] = J.spread_source(raws, *spread_args(case, own=True))[1]
    return f


def longest_path(case: Case) -> int:
    """Slots on the longest acyclic path from the entry program's first slot: back jumps are not
    followed, a BPF-to-BPF call adds its callee's path, a tail call continues in the longest
    program of the prog array that is not yet on the path."""
    import functools
    import sys

    sys.setrecursionlimit(10000)
    progs = [raw for _, raw, _ in case.progs]
    targets = sorted({pi for _, _, pi in case.prog_array})

    def decode(raw, i):
        op, regs = raw[8 * i], raw[8 * i + 1]
        off = int.from_bytes(raw[8 * i + 2:8 * i + 4], "little", signed=True)
        imm = int.from_bytes(raw[8 * i + 4:8 * i + 8], "little", signed=True)
        return op, regs >> 4, off, imm

    def prog_len(pi, on_path):
        raw = progs[pi]
        n = len(raw) // 8

        @functools.lru_cache(maxsize=None)
        def walk(i):
            if i >= n:
                return 0
            op, src, off, imm = decode(raw, i)
            cls, code = op & 7, op & 0xF0
            if op == (A.LD | A.IMM | A.DW):
                return 1 + walk(i + 2)
            if cls in (A.JMP, A.JMP32):
                if code == A.EXIT:
                    return 1
                if code == A.CALL:
                    if src == A.PSEUDO_CALL:
                        return 1 + walk(i + 1 + imm) + walk(i + 1)
                    if imm == A.FN_TAIL_CALL:
                        nxt = [prog_len(t, on_path | {pi}) for t in targets if t not in on_path and t != pi]
                        return 1 + max([walk(i + 1)] + nxt)
                    return 1 + walk(i + 1)
                if code == A.JA:
                    return 1 + (walk(i + 1 + off) if off >= 0 else 0)
                return 1 + max(walk(i + 1), walk(i + 1 + off) if off >= 0 else 0)
            return 1 + walk(i + 1)

        return walk(0)

    return prog_len(0, frozenset())


def oracle_quality(case: Case, batch=None) -> Dict[str, float]:
    """The case's batch on the CPU oracle: share of runs ending with status 0, mean steps over the
    longest acyclic path, distinct R0 values among the finished runs."""
    from harness import run_oracle

    b = batch or make_batch(case)
    o = run_oracle(case.scenario(), b["buf"], b["off"], b["lens"], b["cpu"], headroom=b["headroom"], tailroom=b["tailroom"],
                   step_budget=STEP_BUDGET)
    ok = np.asarray(o["status"]) == 0
    return {"ok": float(ok.mean()), "steps_over_path": float(np.asarray(o["steps"]).mean()) / max(longest_path(case), 1),
            "distinct_r0": int(len(np.unique(np.asarray(o["r0"])[ok])))}
