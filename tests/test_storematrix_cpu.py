"""bpf_skb_store_bytes on the CPU: the model of tests/storematrix.py against hand-worked cases and
against the oracle, and what the JIT generates for a call 9 (no GPU).

* hand KATs of the model, one or more per step of linuxHelperSKBStoreBytes
  (tests/golden/storematrix_kat.json);
* the twin check: the oracle has no helper 9, so for in-frame stores of a fixed length the program with
  the call replaced by byte loads through R3 and byte stores through ctx->data + R2 - 32 must give, on
  the oracle, exactly the packet memory, R0 and steps the model predicts for the helper form -- which
  ties the model's offset base (32 = the frame's first byte), its big-endian read-back and its step
  count to the oracle;
* the generated source: the inline form and its two off-switches, the cold call, the deferral with
  R1-R4 stored, no early load above a call 9, no key store elided in front of one, never spread;
* the register budget of prog_skb_rewrite's kernel."""
import json
import os

import numpy as np
import pytest

import storematrix as SM
from harness import Scenario, kernel_of, run_sequence_oracle
from mimic_amd import asm as A
from mimic_amd import jit as J
from mimic_amd import workloads as W

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "storematrix_kat.json")))["cases"]
FORM = {f.name: f for f in SM.forms()}


def _ptr(x):
    return 0 if x == 0 else SM.Ptr(x[0], x[1])


@pytest.mark.parametrize("case", KAT, ids=[c["name"] for c in KAT])
def test_model_hand_kats(case):
    frame = bytes(0x40 + k for k in range(64))
    st = SM.State(frame, SM.map_bytes())
    for off, hx in case["stack"]:
        b = bytes.fromhex(hx)
        st.stack[off:off + len(b)] = b
    want = bytearray(32) + bytearray(frame) + bytearray(64)
    for off, hx in case["changes"]:
        b = bytes.fromhex(hx)
        want[off:off + len(b)] = b
    got = st.store_bytes(_ptr(case["r1"]), int(case["r2"], 0), _ptr(case["r3"]), int(case["r4"], 0))
    assert got == case["status"], f"{case['name']} ({case['ref']}): status {got}"
    assert bytes(st.pkt) == bytes(want), f"{case['name']} ({case['ref']}): packet memory"


def test_model_call_leaves_registers_and_sets_r0():
    """A failing call is a step that leaves every register: R0 keeps the tag the program put there, and
    the straight-line program has run call_pc + 1 slots.  A successful one runs to the exit."""
    import random

    f = FORM["off_n8"]
    ok = SM.run_process(SM.decode(f.raw), SM.frame(64, SM.H + 8, random.Random(1)), SM.map_bytes())
    bad = SM.run_process(SM.decode(f.raw), SM.frame(64, 500, random.Random(1)), SM.map_bytes())
    assert ok[0] == 0 and ok[3] == -1 and ok[2] == len(SM.decode(f.raw)) - 2
    assert bad[:4] == (SM.BOUNDS, SM.R0_TAG + 500, f.call_pc + 1, f.call_pc)
    assert ok[4][SM.H + 8:SM.H + 16] == SM.PAT.to_bytes(8, "little") and bad[4][SM.H + 8:SM.H + 16] != ok[4][SM.H + 8:SM.H + 16]


def test_twins_on_the_oracle():
    """Byte-wise ldx / stx twins of five in-frame stores (n <= 8) on the oracle against the model of
    the helper form: packet memory, R0, err_pc, and steps less the twin's 2 n extra slots."""
    fs = list(SM.TWINS)
    sc = Scenario(vcpus=SM.V_CPUS, maps=[SM.MAP], progs=[(f.name, f.twin_raw, []) for f in fs])
    rs = [dict(SM._batch_of(f, 99 + k, 64), entry=k) for k, f in enumerate(fs)]
    outs = run_sequence_oracle(sc, rs)[0]
    for k, f in enumerate(fs):
        assert 0 < f.n <= 8 and f.fixed_r2 >= SM.H and f.fixed_r2 + f.n <= SM.H + min(SM.FRAME_LENS)
        want, got = SM.model_batch(f, rs[k], SM.map_bytes()), outs[k]
        assert (np.asarray(got["status"]) == 0).all() and (want["status"] == 0).all(), f.name
        assert np.array_equal(np.asarray(got["r0"]).astype(np.uint64), want["r0"]), f.name
        assert np.array_equal(np.asarray(got["steps"]).astype(np.int64) - f.twin_extra_steps, want["steps"]), f.name
        assert np.array_equal(np.asarray(got["err_pc"]).astype(np.int64), want["err_pc"]), f.name
        assert np.array_equal(got["pkt"], want["pkt"]), f.name


def test_oracle_has_no_helper_9():
    """Why the model: the frozen oracle answers the call with its engine-helper error."""
    f = FORM["off_n8"]
    o = run_sequence_oracle(SM.scenario([f]), [dict(SM._batch_of(f, 5, 8), entry=0)])[0][0]
    assert (np.asarray(o["status"]) == 24).all() and (np.asarray(o["err_pc"]) == f.call_pc).all()


def test_corpus_reaches_every_status_and_edge():
    """The batches hold what the issue lists: every status of the helper, both rooms written, the
    truncated offset, the inline cap's neighbours."""
    assert {SM.FAST_MAX - 1, SM.FAST_MAX, SM.FAST_MAX + 1, 0, 1, 7, 8, 9, 63, 64, 65} <= set(SM.CONST_N)
    seen = set()
    for k, f in enumerate(SM.forms()):
        w, b = SM.expected(k), SM.batch(k)
        seen |= set(int(s) for s in np.unique(w["status"]))
        assert (w["status"] == 0).sum() >= 64 and (w["status"] != 0).sum() >= 16, f.name
        assert (w["r0"][w["status"] != 0] != 0).all(), f"{f.name}: a failing call keeps a non-zero R0"
        if f.arg == "r2":
            assert ((b["arg"] == (1 << 32) + 40) & (w["status"] == 0)).any(), f.name
    assert seen == {SM.OK, SM.BOUNDS, SM.HELPER_VALUE, SM.CTX_ACCESS, SM.PANIC_SLICE}
    w, b = SM.expected(SM.forms().index(FORM["off_n8"])), SM.batch(SM.forms().index(FORM["off_n8"]))
    rooms = 0
    for k in range(SM.N_PACKETS):
        o, L = int(b["off"][k]), int(b["lens"][k])
        rooms |= 1 if w["pkt"][o:o + SM.H].any() else 0
        rooms |= 2 if w["pkt"][o + SM.H + L:o + SM.H + L + SM.T].any() else 0
    assert rooms == 3, "stores into the headroom and into the tailroom"


# ---------------------------------------------------------------------------------------------
# the generated source
# ---------------------------------------------------------------------------------------------
def _src(fs, **env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return J.kernel_source(*kernel_of(SM.scenario(fs), J.CTX_SKB))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def test_source_constant_length_site_is_inline():
    """Fails on a build without the helper: predecode turned the call into TERM(MIMIC_ERR_ENGINE_HELPER)."""
    src = _src([FORM["off_n8"]])
    assert "store_bytes_fast<8u>(kp, L, SK_, r1, r2, r3, r4, r0)" in src and "COLD_CALL(cold_store_bytes(kp, sp_)" in src
    assert f"TERM(24, {FORM['off_n8'].call_pc})" not in src
    for n in (SM.FAST_MAX, SM.FAST_MAX + 1, 0):
        s = _src([FORM[f"off_n{n}"]])
        assert ("store_bytes_fast" in s) == (0 < n <= SM.FAST_MAX) and "cold_store_bytes" in s, n


@pytest.mark.parametrize("knob", ["MIMIC_JIT_SKBSTORE", "MIMIC_JIT_FAST"])
def test_source_off_switches(knob):
    src = _src([FORM["off_n8"]], **{knob: "0"})
    assert "store_bytes_fast" not in src and "COLD_CALL(cold_store_bytes(kp, sp_)" in src


def test_source_register_length_site_is_cold_only():
    src = _src([FORM["len_reg"]])
    assert "store_bytes_fast" not in src and "COLD_CALL(cold_store_bytes(kp, sp_)" in src


def test_source_xdp_kernel_has_no_inline_form():
    raw = A.assemble([A.mov64_imm(2, 0), A.mov64_reg(3, 10), A.mov64_imm(4, 4), A.call(A.FN_SKB_STORE_BYTES), A.exit_()])[0]
    src = J.kernel_source([raw], J.CTX_XDP)
    assert "store_bytes_fast" not in src and "cold_store_bytes" in src


def test_source_chunk_kernels_defer_with_r1_to_r4():
    """The four-program kernels have more slow-path sites than the JIT inlines: a call 9 that misses its
    inline form is deferred, and the site stores what helper_skb_store_bytes reads when the resume
    kernel runs it (analyze_live: R1-R4), R0 and R10."""
    import re

    for first, fs in SM.chunks():
        src = _src(fs)
        assert "L_defer:" in src and "COLD_CALL(cold" not in src, fs[0].name
        for k, f in enumerate(fs):
            site = [l for l in src.splitlines() if f"DFR({f.call_pc}u, {k}u)" in l]
            assert len(site) == 1, f.name
            stored = set(int(x) for x in re.findall(r"dr_->r\[(\d+)\]", site[0]))
            assert {0, 1, 2, 3, 4, 10} <= stored, (f.name, site[0])


def test_source_census_counts_the_call_as_a_store():
    src = _src([FORM["len_reg"]], MIMIC_JIT_CENSUS="1")
    assert "COLD_CALL_K(4, cold_store_bytes(kp, sp_)" in src


def test_source_no_early_load_above_the_call():
    """analyze_spec: every H_CALL is a barrier.  The barrier form's LD_ABS after the call (a branch in
    between makes it an early load) is issued after the call's line, the one before it is not early."""
    f = FORM["barrier"]
    lines = _src([f]).splitlines()
    call = [i for i, l in enumerate(lines) if "cold_store_bytes(kp, sp_)" in l]
    early = [i for i, l in enumerate(lines) if "// early LD_ABS for slot" in l]
    assert len(call) == 1 and early, "the form has early loads"
    assert min(early) > call[0], "an early packet load above bpf_skb_store_bytes"
    slots = [int(l.rsplit("slot", 1)[1]) for l in lines if "// early LD_ABS for slot" in l]
    assert min(slots) > f.call_pc


def test_source_key_store_in_front_of_the_call_is_made():
    """analyze_elide gives up on a helper that reads the stack: the lookup's key store in the map
    form is made where it stands, not deferred into the lookup's cold path."""
    src = _src([FORM["src_map_n8"]])
    assert "key store deferred" not in src
    plain = W.prog_classifier()
    assert "key store deferred" in J.kernel_source([plain.raw], J.CTX_XDP), "the analysis still elides without a call 9"


def test_never_spread():
    """A program set that calls helper 9 runs one lane per vCPU (analyze_spread refuses the call)."""
    cls = W.prog_classifier()
    progs = [(cls.raw, cls.relocs)]
    spec = J.spread_spec(progs, cls.maps, 1024)
    assert J.spread_source([cls.raw], *spec)[1] is True
    items = [A.mov64_reg(6, 1), A.mov64_reg(3, 10), A.alu64("add", 3, -8), A.mov64_imm(2, 0), A.mov64_imm(4, 4),
             A.call(A.FN_SKB_STORE_BYTES), A.mov64_reg(1, 6)]
    raw9 = A.assemble(items)[0] + cls.raw
    rel9 = [(s + len(items), n) for s, n in cls.relocs]
    spec9 = J.spread_spec([(raw9, rel9)], cls.maps, 1024)
    assert spec9[0], "the spread request still names the map"
    assert J.spread_source([raw9], *spec9)[1] is False


def test_rewrite_programs_on_the_oracle_and_budget():
    """prog_skb_rewrite_direct on the oracle equals workloads.skb_rewrite_expected where the context
    loaded; prog_skb_rewrite's kernel (hipRTC, gfx950) has its four sites inline and no scratch."""
    from harness import run_oracle_skb

    d = W.prog_skb_rewrite_direct()
    buf, off, lens = W.make_skb_packets(2048, sizes=SM.FRAME_LENS, weights=(1,) * 5, variety=0.3)
    cpu = (np.arange(2048) % 64).astype(np.int32)
    o = run_oracle_skb(Scenario(vcpus=64, progs=[(d.name, d.raw, d.relocs)]), buf, off, lens, cpu)
    exp, r0 = W.skb_rewrite_expected(buf, off, lens)
    ok = np.asarray(o["status"]) == 0
    assert ok.sum() > 1500 and (~ok).sum() > 50 and (r0[ok] > 0).sum() > 1000
    assert np.array_equal(np.asarray(o["r0"]).astype(np.uint64)[ok], r0[ok])
    for i in range(2048):
        a, b = int(off[i]), int(off[i]) + 96 + int(lens[i])
        assert np.array_equal(o["pkt"][a:b], exp[a:b] if ok[i] else buf[a:b]), i
    p = W.prog_skb_rewrite()
    src = J.kernel_source([p.raw], J.CTX_SKB)
    assert src.count("store_bytes_fast<6u>") == 2 and "store_bytes_fast<2u>" in src and "store_bytes_fast<1u>" in src
    r = J.kernel_resources(J.code_object(src))
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["agpr"] == 0 and r["waves_per_simd"] >= 2, r


def test_inline_cap_is_one_number():
    """The inline form's cap stands in runtime.h (SKB_STORE_FAST_MAX, which store_bytes_fast asserts), in
    jit.cpp (kStoreFastMax, which decides whether a site gets the form) and in the corpus (FAST_MAX, whose
    neighbours the forms are built at): the three are equal, and the generator takes a site at the cap
    and leaves the one past it."""
    import re

    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mimic_amd", "csrc")
    rt = int(re.search(r"#define SKB_STORE_FAST_MAX (\d+)u", open(os.path.join(csrc, "runtime.h")).read()).group(1))
    gen = int(re.search(r"kStoreFastMax = (\d+);", open(os.path.join(csrc, "jit.cpp")).read()).group(1))
    assert rt == gen == SM.FAST_MAX
    assert f"store_bytes_fast<{rt}u>" in _src([FORM[f"off_n{rt}"]]) and "store_bytes_fast" not in _src([FORM[f"off_n{rt + 1}"]])


def test_interpreter_instances_with_the_helper_do_not_spill():
    """Register budget of the interpreter instances that carry helper_skb_store_bytes, read from the built
    library like tests/test_interp_regs.py does for the batch kernel: mimic_xdp_store_kernel (the batch
    body with the helper, at the compiler's own budget) keeps 3 waves per SIMD and spills nothing; the
    step and resume kernels keep their waves.  The batch kernel without it is test_interp_regs.py's."""
    import test_interp_regs as R

    r = R._kernel("mimic_xdp_store_kernel")
    assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["agpr"] == 0, r
    assert r["vgpr_total"] <= 168 and r["waves_per_simd"] >= 3, r
    assert R._kernel("mimic_xdp_resume_kernel")["waves_per_simd"] >= 3 and R._kernel("mimic_xdp_step_kernel")["waves_per_simd"] >= 2
