"""Gates on the structured fuzz corpus (tests/fuzz_struct.py), on the CPU host only.

The GPU parity tests (test_gpu_fuzz_struct.py) are only as good as the programs they run, so the
corpus itself is checked here, on the oracle and on the generated kernel source -- never on the
engine's results:

* the programs finish (status 0), run most of their slots and return many different R0 values;
* every analysis of jit.cpp fires in at least 8 programs and is refused in at least 4 neighbours
  the generator marked "must refuse";
* what the generator intended for a case (`Case.expect`) is what the JIT decided.  A disagreement
  means the generator's model of a precondition is wrong, or the analysis is unsound or
  needlessly narrow (DESIGN.md 3.2 lists the ones found so far);
* every kernel of the corpus generates (default, spread and owned forms), a subset compiles.
"""
import functools
import hashlib

import numpy as np
import pytest

import fuzz_struct as F
from mimic_amd import jit as J

SEEDS = range(F.N_SEEDS)


@functools.lru_cache(maxsize=None)
def _case(seed):
    return F.generate(seed)


@functools.lru_cache(maxsize=None)
def _features(seed):
    return F.source_features(_case(seed))


@functools.lru_cache(maxsize=None)
def _quality(seed):
    return F.oracle_quality(_case(seed))


def test_corpus_size_and_determinism():
    assert F.N_SEEDS >= 64
    h = hashlib.sha256()
    for s in SEEDS:
        a, b = F.generate(s), F.generate(s)
        assert a.progs == b.progs and a.maps == b.maps and a.map_init == b.map_init and a.vcpus == b.vcpus
        ba, bb = F.make_batch(a), F.make_batch(b)
        assert all(np.array_equal(ba[k], bb[k]) for k in ("buf", "off", "lens", "cpu")) and ba["sched"] == bb["sched"]
        for _, raw, rel in a.progs:
            h.update(raw)
            h.update(repr(rel).encode())
        h.update(ba["buf"].tobytes())
        h.update(ba["cpu"].tobytes())
    # the corpus is part of the record, like the seeds of fuzz.py: a change of the generator that
    # moves it shows here (update the digest together with DESIGN.md 5's corpus rows)
    assert h.hexdigest() == CORPUS_SHA256, h.hexdigest()


CORPUS_SHA256 = "1907e8f4e77a82737995cfb56b0f9e9aef68b8e6d38375a9be5256f961211f85"


def test_batches_have_the_required_shape():
    scheds, rooms = set(), 0
    for s in SEEDS:
        c, b = _case(s), F.make_batch(_case(s))
        assert len(b["lens"]) == F.N_PACKETS == 1000 and c.vcpus in (1, 7, 64)
        assert set(np.unique(b["lens"]).tolist()) <= set(F.LENGTHS)
        assert int(b["cpu"].min()) >= 0 and int(b["cpu"].max()) < c.vcpus
        scheds.add(b["sched"])
        rooms += not np.isscalar(b["headroom"])
    assert scheds == {"explicit", "chunked", "interleaved"}
    assert abs(rooms - F.N_SEEDS / 3) <= 1
    assert {_case(s).vcpus for s in SEEDS} == {1, 7, 64}


def test_programs_that_write_shared_maps_run_on_one_vcpu():
    n = 0
    for s in SEEDS:
        c = _case(s)
        if c.shared_write:
            n += 1
            assert c.vcpus == 1
    assert n >= 4


def test_programs_finish():
    ok = [_quality(s)["ok"] for s in SEEDS]
    assert float(np.mean(ok)) >= 0.90, float(np.mean(ok))
    assert min(ok) >= 0.50, [(s, ok[s]) for s in SEEDS if ok[s] < 0.5]


def test_programs_run_most_of_their_slots():
    short = [(s, round(_quality(s)["steps_over_path"], 2)) for s in SEEDS if _quality(s)["steps_over_path"] < 0.60]
    assert not short, short


def test_programs_return_many_values():
    many = sum(_quality(s)["distinct_r0"] >= 8 for s in SEEDS)
    assert many >= 0.75 * F.N_SEEDS, many


@pytest.mark.parametrize("feature", F.FEATURES)
def test_every_analysis_fires_and_is_refused(feature):
    fires = [s for s in SEEDS if _features(s)[feature]]
    refused = [s for s in SEEDS if _case(s).base_seed is not None and _case(s).expect.get(feature) is False
               and not _features(s)[feature]]
    assert len(fires) >= 8, (feature, fires)
    assert len(refused) >= 4, (feature, refused)


@pytest.mark.parametrize("seed", SEEDS)
def test_intent_matches_the_jit(seed):
    c, f = _case(seed), _features(seed)
    wrong = {k: (want, f[k]) for k, want in c.expect.items() if f[k] != want}
    assert not wrong, f"seed {seed} ({c.family}, neighbour {c.neighbour}, blocks {c.blocks}): feature -> (intended, JIT) {wrong}"


def test_neighbours_flip_what_they_are_meant_to_flip():
    """Every neighbour is another program than its base and differs from it in at least one intended
    decision -- or is one of the steps that must leave every decision as it is (F.STILL_ACCEPT: same
    expectations as the base, which test_intent_matches_the_jit then holds the JIT to)."""
    n = 0
    for s in SEEDS:
        c = _case(s)
        if c.base_seed is None:
            continue
        n += 1
        base = _case(c.base_seed)
        assert base.neighbour is None and base.family == c.family
        assert c.progs != base.progs
        if c.neighbour in F.STILL_ACCEPT or (c.neighbour == "alu32_on_8" and c.maps[0]["value_size"] != 8):
            assert all(base.expect.get(k) == v for k, v in c.expect.items()), (s, c.neighbour)
        else:
            assert any(k in base.expect and base.expect[k] != v for k, v in c.expect.items()), (s, c.neighbour)
    assert n >= 40


def test_called_functions_really_run():
    """A BPF-to-BPF call lands one slot before its target (quirk Q12): a function without a pad slot
    in front of its label starts on the EXIT before it and returns at once (what the
    `calls_land_on_exit` neighbours do on purpose).  One packet of every
    set with calls is stepped on the oracle: each call site is followed by the callee's first slots."""
    from harness import build_oracle
    from oracle.pyoracle import OracleProcess

    n = 0
    for s in SEEDS:
        c = _case(s)
        if not any(b.startswith("call") for b in c.blocks):
            continue
        raw = c.progs[0][1]
        vm, _, pids = build_oracle(c.scenario())
        p = OracleProcess(vm, pids[0], xdp=(bytes(64), 0, 0, 0, 0, 0))
        p.set_cpu(0)
        trace = []
        while len(trace) < F.STEP_BUDGET:
            trace.append(p.pc())
            if p.step()[0] != 0:
                break
        p.cleanup()
        vm.close()
        calls = [k for k, pc in enumerate(trace) if raw[8 * pc] == 0x85 and raw[8 * pc + 1] >> 4 == 1]
        assert len(calls) >= sum(b.startswith("call") for b in c.blocks), (s, calls)
        for k in calls:
            pc = trace[k]
            pad = pc + int.from_bytes(raw[8 * pc + 4:8 * pc + 8], "little", signed=True)
            if c.neighbour == "calls_land_on_exit":     # the unpadded neighbours: on an EXIT, and back at once
                assert raw[8 * pad] == 0x95 and trace[k + 1:k + 3] == [pad, pc + 1], (s, pc, trace[k:k + 3])
            else:
                assert trace[k + 1:k + 4] == [pad, pad + 1, pad + 2], (s, pc, trace[k:k + 4])
        n += 1
    assert n >= 4


def test_deferral_follows_the_site_count():
    for s in SEEDS:
        c = _case(s)
        if "defer" in c.expect:
            assert (F.site_count(c) > 48) == c.expect["defer"], (s, F.site_count(c))


def test_every_corpus_kernel_generates():
    n = 0
    for s in SEEDS:
        c = _case(s)
        raws, ctx, vc = F.kernel_args(c)
        assert "mimic_jit_kernel" in J.kernel_source(raws, ctx, vc)
        for own in (False, True):
            src, ok = J.spread_source(raws, *F.spread_args(c, own=own))
            assert "mimic_jit_kernel" in src
            assert ("#define MIMIC_SPREAD 1" in src) == ok and ("#define MIMIC_SPREAD_OWN 1" in src) == (ok and own)
            n += ok
    assert n >= 16


def test_large_sets_defer_natively():
    """The sets with more than 48 slow-path sites run JIT -> resume kernel in test_gpu_fuzz_struct.py's
    test_default_jit: no call is left in their kernels."""
    big = [s for s in SEEDS if _case(s).expect.get("defer")]
    assert len(big) >= 8
    for s in big:
        src = J.kernel_source(*F.kernel_args(_case(s)))
        assert "L_defer:" in src and "COLD_CALL(cold" not in src


# single-program focused cases: the corpus's small kernels (a chain is several programs behind one
# dispatch block; seed 52's three programs spill 98 VGPRs at the 4-wave budget)
COMPILE_SEEDS = [s for s in SEEDS if _case(s).base_seed is None and _case(s).family in ("counter", "loads", "hash", "stack")][::3][:8]


@pytest.mark.parametrize("seed", COMPILE_SEEDS)
def test_small_corpus_kernels_compile_within_budget(seed):
    """hipRTC builds for gfx950 of focused cases (inlined slow paths: built for 4 waves per SIMD):
    the budget test_jit_cpu.py holds cfg 4's kernel to -- at most 128 unified VGPRs, 4 waves, at
    most 64 spilled VGPRs."""
    c = _case(seed)
    assert len(COMPILE_SEEDS) == 8 and F.site_count(c) <= 48
    r = J.kernel_resources(J.code_object(J.kernel_source(*F.kernel_args(c))))
    assert r["vgpr_total"] <= 128 and r["waves_per_simd"] >= 4 and r["vgpr_spill"] <= 64, r


def test_deferred_key_store_is_made_before_a_generic_lookup():
    """Seeds 45 / 47 / 49 / 51 (hash lookups whose LD_IMM64 sits in an earlier block): the key store
    was deferred by analyze_elide, but the call went straight to the generic helper, which reads
    the key from the stack.  The store now precedes it."""
    for s in SEEDS:
        c = _case(s)
        if not (c.family == "hash" and c.neighbour == "ldimm_other_block"):
            continue
        src = J.kernel_source(*F.kernel_args(c))
        assert _features(s)["elide"]
        k = src.index("cold_lookup(kp, sp_)")
        before = src[src.rindex("steps++;", 0, k):k]
        assert "stack_store(" in before and "fwd0_" in before, before
