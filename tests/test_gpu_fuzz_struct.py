"""The structured fuzz corpus (tests/fuzz_struct.py) on MI355X against the oracle, on every kernel
form: the default JIT and the batch interpreter for every seed; the spread (table) and owned forms
for every set analyze_spread accepts, and forced spread on the neighbours it must refuse; three
batches in one owned launch (RunXDPMany); deferred slow paths (the large sets natively, eight small
ones with the cold paths forced to defer); eight seeds with the fast paths off.  Each run compares
per-packet R0 / status / steps / err_pc, the packet memory and every map byte, bit for bit.

test_fuzz_struct_cpu.py gates the corpus itself (the programs finish, every analysis fires and is
refused, the generator's intent matches the JIT's decisions)."""
import functools

import numpy as np
import pytest

import fuzz_struct as F
import mimic_amd as M
from harness import (assert_same, build_engine, build_oracle, kernel_of, ncpus, run_engine, run_oracle, spread_kernel_of)
from mimic_amd import jit as J

pytestmark = pytest.mark.gpu

SEEDS = list(range(F.N_SEEDS))


@functools.lru_cache(maxsize=None)
def _case(seed):
    return F.generate(seed)


@functools.lru_cache(maxsize=None)
def _spread_ok(seed):
    """What analyze_spread says; without a built library (a collection of the whole suite before
    build()) the generator's intent, so that the module still collects and deselects."""
    c = _case(seed)
    try:
        return J.spread_source([raw for _, raw, _ in c.progs], *F.spread_args(c))[1]
    except OSError:
        return c.expect.get("spread") is True


SPREAD = [s for s in SEEDS if _spread_ok(s)]
REFUSED = [s for s in SEEDS if _case(s).expect.get("spread") is False]
UNPADDED = [s for s in SEEDS if _case(s).neighbour == "calls_land_on_exit"]
# sets whose generic paths really run: stack accesses through a copy of R10, map_update / map_delete,
# generic hash lookups (small enough to inline their slow paths: here they are forced to defer)
DEFER_SMALL = ([s for s in SEEDS if _case(s).family == "stack"][:4] +
               [s for s in SEEDS if _case(s).family == "hash" and _case(s).neighbour is None][-2:] +
               [s for s in SEEDS if _case(s).family == "general" and F.site_count(_case(s)) <= 48][:2])
FAST_OFF = [s for s in SEEDS if _case(s).base_seed is None][::max(1, len(SEEDS) // 14)][:8]


def jit_kernels():
    ks = [kernel_of(_case(s).scenario()) for s in SEEDS]
    for s in SPREAD:
        ks += [spread_kernel_of(_case(s).scenario()), spread_kernel_of(_case(s).scenario(), own=True)]
    return ks


def _mode(sched):
    return {"explicit": M.SCHED_EXPLICIT, "chunked": M.SCHED_CHUNKED, "interleaved": M.SCHED_INTERLEAVED}[sched]


@functools.lru_cache(maxsize=None)
def _reference(seed, sched=None):
    """(batch, oracle result) of a seed, computed once; sched: an implicit schedule instead of the
    seed's own (spread launches need one).  Tests only read it."""
    c = _case(seed)
    b = F.make_batch(c, sched=sched)
    o = run_oracle(c.scenario(), b["buf"], b["off"], b["lens"], b["cpu"], headroom=b["headroom"], tailroom=b["tailroom"],
                   step_budget=F.STEP_BUDGET)
    return b, o


def _engine(seed, b, **kw):
    c = _case(seed)
    return run_engine(c.scenario(), b["buf"], b["off"], b["lens"], b["cpu"] if b["sched"] == "explicit" else None,
                      headroom=b["headroom"], tailroom=b["tailroom"], step_budget=F.STEP_BUDGET, schedule=_mode(b["sched"]), **kw)


def _same(b, o, e):
    if np.isscalar(b["headroom"]):
        assert_same(o, e)
        return
    # per-packet rooms: the packet memories (the gaps between them are not process memory)
    H, T = b["headroom"], b["tailroom"]
    for i in range(len(b["lens"])):
        a, m = int(b["off"][i]), int(H[i]) + int(b["lens"][i]) + int(T[i])
        assert bytes(o["pkt"][a:a + m]) == bytes(e["pkt"][a:a + m]), f"packet {i} memory differs"
    assert_same(o, e, check_pkt=False)


def _implicit(seed):
    s = F.make_batch(_case(seed))["sched"]
    return s if s != "explicit" else "interleaved"


@pytest.mark.parametrize("seed", SEEDS)
def test_default_jit(gpu, seed):
    b, o = _reference(seed)
    e = _engine(seed, b, spread=0)
    assert e["last_exec"] == "jit"
    _same(b, o, e)


@pytest.mark.parametrize("seed", SEEDS)
def test_interpreter(gpu, seed):
    b, o = _reference(seed)
    e = _engine(seed, b, exec_mode="interp")
    assert e["last_exec"] == "interp"
    _same(b, o, e)


@pytest.mark.parametrize("seed", SPREAD)
def test_spread_forced(gpu, seed, monkeypatch):
    monkeypatch.setenv("MIMIC_SPREAD_OWN", "0")     # the table form (the owned form: below)
    b, o = _reference(seed, _implicit(seed))
    e = _engine(seed, b, spread=1)
    assert e["last_exec"] == "spread"
    _same(b, o, e)
    assert e["steps_total"] == int(np.asarray(o["steps"]).astype(np.int64).sum())


@pytest.mark.parametrize("seed", SPREAD)
def test_owned_form(gpu, seed):
    b, o = _reference(seed, _implicit(seed))
    per_vcpu = int(np.bincount(b["cpu"]).max())
    assert 2 <= per_vcpu <= 256
    e = _engine(seed, b, spread=1)
    assert e["last_exec"] == "spread_own"
    _same(b, o, e)
    assert e["steps_total"] == int(np.asarray(o["steps"]).astype(np.int64).sum())


@pytest.mark.parametrize("seed", REFUSED)
@pytest.mark.parametrize("own", ["0", "1"])
def test_refused_neighbours_stay_on_one_lane_per_vcpu(gpu, seed, own, monkeypatch):
    monkeypatch.setenv("MIMIC_SPREAD_OWN", own)
    b, o = _reference(seed, _implicit(seed))
    e = _engine(seed, b, spread=1)
    assert e["last_exec"] == "jit"
    _same(b, o, e)


@pytest.mark.parametrize("seed", SPREAD)
def test_three_batches_one_owned_launch(gpu, seed):
    """RunXDPMany: three batches of one shape in one launch of the owned kernel, against the
    oracle running them one after another on one VM (as test_gpu_many.py does)."""
    c = _case(seed)
    sc = c.scenario()
    sched = _implicit(seed)
    batches = [F.make_batch(c, salt=1 + k, sched=sched, rooms=False) for k in range(3)]
    ovm, omids, opids = build_oracle(sc)
    outs = []
    for b in batches:
        buf = b["buf"].copy()
        o = ovm.run_xdp_batch(opids[0], buf, b["off"], b["lens"], b["cpu"], 0, 0, None, None, None, F.STEP_BUDGET)
        o["pkt"] = buf
        outs.append(o)
    omaps = {m["name"]: [ovm.map_values(omids[m["name"]], k) for k in range(ncpus(sc, m))] for m in sc.maps}
    ovm.close()
    vm, maps, pids = build_engine(sc, spread=1)
    dev = [M.XDPBatch.from_numpy(b["buf"], b["off"], b["lens"], device="cuda:0", schedule=_mode(sched), step_budget=F.STEP_BUDGET)
           for b in batches]
    res = vm.RunXDPMany(pids[0], dev)
    assert vm.LastExec() == "spread_own"
    for k, (o, r, d) in enumerate(zip(outs, res, dev)):
        e = r.numpy(F.N_PACKETS)
        for f in ("r0", "status", "steps", "err_pc"):
            x = np.asarray(o[f]).astype(np.uint64 if f == "r0" else np.int64)
            y = np.asarray(e[f]).astype(np.uint64 if f == "r0" else np.int64)
            bad = np.nonzero(x != y)[0]
            assert len(bad) == 0, f"batch {k} {f} differs at {bad[:6]}: oracle={x[bad[:6]]} engine={y[bad[:6]]}"
        assert np.array_equal(o["pkt"], d.pkt_data.cpu().numpy()), f"batch {k} packet memory"
    for m in sc.maps:
        for k in range(ncpus(sc, m)):
            assert maps[m["name"]].Values(k) == omaps[m["name"]][k], f"map {m['name']} cpu {k}"
    vm.close()


@pytest.mark.parametrize("seed", DEFER_SMALL)
def test_small_sets_with_deferred_slow_paths(gpu, seed, monkeypatch):
    """The same programs that test_default_jit runs with inlined slow paths, through the resume
    kernel.  The knob is read when the kernel is generated, which the session prewarm does in
    its own pass before any test: these few kernels are compiled here."""
    monkeypatch.setenv("MIMIC_JIT_COLD", "defer")
    src = J.kernel_source(*F.kernel_args(_case(seed)))
    assert "L_defer:" in src and "DFR(" in src and "COLD_CALL(cold" not in src
    b, o = _reference(seed)
    e = _engine(seed, b, spread=0)
    assert e["last_exec"] == "jit"
    _same(b, o, e)


@pytest.mark.parametrize("seed", FAST_OFF)
def test_fast_paths_off(gpu, seed, monkeypatch):
    """MIMIC_JIT_FAST=0: every access through the generic path, no analysis: a difference that is
    only there with the fast paths on is an analysis's, not runtime.h's.  Compiled here (see above)."""
    monkeypatch.setenv("MIMIC_JIT_FAST", "0")
    src = J.kernel_source(*F.kernel_args(_case(seed)))
    assert "counter increment of" not in src and "issued early" not in src and "fwd0_" not in src
    b, o = _reference(seed)
    e = _engine(seed, b, spread=0)
    assert e["last_exec"] == "jit"
    _same(b, o, e)



def _fast_off(c, monkeypatch):
    monkeypatch.setenv("MIMIC_JIT_FAST", "0")
    b = F.make_batch(c)
    sc = c.scenario()
    o = run_oracle(sc, b["buf"], b["off"], b["lens"], b["cpu"], headroom=b["headroom"], tailroom=b["tailroom"],
                   step_budget=F.STEP_BUDGET)
    e = run_engine(sc, b["buf"], b["off"], b["lens"], b["cpu"] if b["sched"] == "explicit" else None, headroom=b["headroom"],
                   tailroom=b["tailroom"], step_budget=F.STEP_BUDGET, schedule=_mode(b["sched"]), spread=0)
    assert e["last_exec"] == "jit"
    _same(b, o, e)


@pytest.mark.parametrize("seed", UNPADDED)
def test_fast_paths_off_calls_landing_on_exit(gpu, seed, monkeypatch):
    """The general cases with BPF-to-BPF calls once more without the functions' pad slots: every call
    lands on the EXIT in front of its target (quirk Q12) and returns at once.  These sets also run on
    every other form above (they are corpus members).

    Seed 93 (435 slots, 290 slow-path sites, six functions, one vCPU) is the finding of DESIGN.md 3.2:
    with the return switch at every EXIT this kernel came back from its second call with the step
    counter and the restored registers wrong (280 / 278 / 279 steps against the oracle's 346 / 320 /
    323 for the first three packets, status 0), while its source read correctly.  Kernels without
    fast paths now send every return through one block per program (jit.cpp ret_dispatch)."""
    _fast_off(_case(seed), monkeypatch)


@pytest.mark.parametrize("nblocks", [19, 20])
def test_fast_paths_off_shortest_known_prefix(gpu, nblocks, monkeypatch):
    """The smallest program known to have shown seed 93's difference: its first 20 blocks (386 slots,
    248 sites), whose 20th block is the fourth call block (the sixth function, the sixth return site).
    With the return switch at every EXIT it differed for 20 blocks (steps 232 / 230 / 231 against
    298 / 272 / 275) and was exact for 19 (366 slots, five return sites), for padded functions, and
    with or without per-packet rooms.  No hand-written program showed it: seven constructed programs
    of two to four unpadded call blocks and up to 180 sites were exact."""
    c = F.prefix_case(82, nblocks, pad=False)
    c.seed = 93
    _fast_off(c, monkeypatch)
