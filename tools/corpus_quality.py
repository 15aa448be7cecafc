#!/usr/bin/env python3
"""How deep does a fuzz corpus reach?  For each of the suite's random-program corpora this runs every
program's batch on the CPU oracle and reads the JIT's decisions from the generated kernel source
(no GPU):

* share of (program, packet) runs that end with status 0, and programs where every packet errs;
* mean steps run as a share of the program set's slots;
* programs whose finished packets return at least 8 distinct R0 values;
* how many programs each analysis of jit.cpp fires in.

Corpora: the xdp fuzz of test_gpu_parity.py (40 seeds of tests/fuzz.py), the hash fuzz of
test_gpu_hash.py (12), the sk_buff fuzz of test_gpu_skb.py (24 seeds of tests/fuzz_skb.py) and the
structured corpus of tests/fuzz_struct.py.  Prints one row per corpus (a Markdown table: DESIGN.md 5).

    python tools/corpus_quality.py
"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from harness import kernel_of, packets_to_buffer, run_oracle, run_oracle_skb, spread_kernel_of  # noqa: E402
from mimic_amd import jit as J  # noqa: E402

FEATURES = ("fwd", "elide", "early", "inc", "vc", "spread", "defer")


def features(sc, ctx=0):
    raws, _, vc = kernel_of(sc, ctx)
    src = J.kernel_source(raws, ctx, vc)
    f = {"fwd": re.search(r"uint32_t fwd\d+_\d+_ = 0;", src) is not None,
         "elide": "key store deferred into the lookup's cold path" in src,
         "early": "issued early" in src,
         "inc": ": counter increment of r" in src,
         "vc": "vc_open(" in src,
         "defer": "L_defer:" in src,
         "spread": False}
    if ctx == 0:
        f["spread"] = J.spread_source(raws, *spread_kernel_of(sc)[3])[1]
    return f


def old_xdp():
    import test_gpu_parity as T

    for seed in range(40):
        sc, rng = T._fuzz(seed)
        pk = [bytes(rng.integers(0, 256, int(rng.choice([0, 14, 60, 64, 100])), dtype=np.uint8)) for _ in range(64)]
        buf, off, lens = packets_to_buffer(pk)
        cpu = rng.integers(0, 8, 64).astype(np.int32)
        yield sc, run_oracle(sc, buf, off, lens, cpu, step_budget=5000), features(sc)


def old_hash():
    import test_gpu_hash as T

    for seed in range(12):      # the batch of test_gpu_hash.py's fuzz test: 48 packets, one vCPU
        sc, rng = T._fuzz(seed)
        pk = [bytes(rng.integers(0, 256, int(rng.choice([0, 14, 64])), dtype=np.uint8)) for _ in range(48)]
        buf, off, lens = packets_to_buffer(pk)
        yield sc, run_oracle(sc, buf, off, lens, np.zeros(len(pk), np.int32), step_budget=4000), features(sc)


def old_skb():
    import test_gpu_skb as T
    from mimic_amd import workloads as W

    for seed in range(24):      # test_gpu_skb.py's test_skb_fuzz
        sc, rng = T._fuzz(seed)
        buf, off, lens = W.make_skb_packets(96, sizes=(14, 40, 64, 128, 576), weights=(1, 1, 3, 2, 1), seed=seed, variety=0.6)
        cpu = rng.integers(0, 8, len(lens)).astype(np.int32)
        yield sc, run_oracle_skb(sc, buf, off, lens, cpu, ifindex=3, step_budget=5000), features(sc, 1)


def structured():
    import fuzz_struct as F

    for seed in range(F.N_SEEDS):
        c = F.generate(seed)
        b = F.make_batch(c)
        sc = c.scenario()
        o = run_oracle(sc, b["buf"], b["off"], b["lens"], b["cpu"], headroom=b["headroom"], tailroom=b["tailroom"],
                       step_budget=F.STEP_BUDGET)
        yield sc, o, features(sc)


def row(name, corpus):
    n = runs = ok = dead = many = 0
    share = []
    fired = {f: 0 for f in FEATURES}
    for sc, o, f in corpus:
        st = np.asarray(o["status"])
        good = st == 0
        n += 1
        runs += len(st)
        ok += int(good.sum())
        dead += not good.any()
        many += len(np.unique(np.asarray(o["r0"])[good])) >= 8
        slots = sum(len(raw) // 8 for _, raw, _ in sc.progs)
        share.append(float(np.asarray(o["steps"]).mean()) / max(slots, 1))
        for k in FEATURES:
            fired[k] += bool(f[k])
    cov = " ".join(f"{k} {fired[k]}" for k in FEATURES)
    return (f"| {name} | {n} | {100.0 * ok / runs:.1f} % | {dead} | {100.0 * float(np.mean(share)):.0f} % | {many} | {cov} |")


def main():
    print("| corpus | programs | runs ending with status 0 | programs where every packet errs | mean steps / slots | "
          "programs with >= 8 distinct R0 | programs each analysis fires in |")
    print("|---|---|---|---|---|---|---|")
    print(row("xdp fuzz (`fuzz.py`, `test_gpu_parity.py`)", old_xdp()))
    print(row("hash fuzz (`fuzz.py`, `test_gpu_hash.py`)", old_hash()))
    print(row("sk_buff fuzz (`fuzz_skb.py`, `test_gpu_skb.py`)", old_skb()))
    print(row("structured (`fuzz_struct.py`)", structured()))


if __name__ == "__main__":
    main()
