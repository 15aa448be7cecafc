"""Time the tc rewrite workload (workloads.prog_skb_rewrite: MAC swap + TTL decrement through
bpf_skb_store_bytes) against the same rewrite with byte stores through ctx->data, on one GPU.

    python tools/skb_store_probe.py [--packets N] [--steps K] [--warmup W] [--rounds R] [--parent LIB] [--out FILE]

One batch of N sk_buff contexts (cfg 5's generator: IMIX frames, V = 128K, interleaved schedule) per
step; ms per batch = device time between two events around K back-to-back launches, after W warm-up
launches of the same VM.  Three runs are compared, alternated R times:

    direct@parent   prog_skb_rewrite_direct on the library --parent names (MIMIC_LIB: a build of the
                    parent commit next to libmimic_amd.so); skipped when the file is not there
    helper          prog_skb_rewrite on this build, default knobs (the inline form store_bytes_fast)
    helper_knob_off prog_skb_rewrite on this build with MIMIC_JIT_SKBSTORE=0 (every call cold)

plus direct on this build.  A library is chosen when it is loaded, so each round starts one child
process per library, one after the other; inside a child the runs alternate.  Both programs read and
write the same packet bytes (the probe checks that on the first batch), so equal HBM traffic is the
expectation; the helper form adds stack traffic.  Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def direct_program():
    """workloads.prog_skb_rewrite_direct, restated here so that the baseline does not depend on this
    tree's workloads.py (it runs on a checkout of the parent commit as it stands): IPv4 frames of at
    least 34 bytes get their MACs swapped, the TTL decremented and the checksum patched
    (ip_decrease_ttl) with byte stores through ctx->data; R0 = the new TTL, 0 for other frames."""
    from mimic_amd import asm as A

    S = A.SKB
    it = [A.mov64_reg(6, 1), A.ldx(4, 2, 6, S["len"]), A.jmp("jlt", 2, 34, "out"),
          A.ld_abs(2, 12), A.jmp("jne", 0, 0x0800, "out"), A.ldx(4, 7, 6, S["data"])]
    for k in range(12):
        it += [A.ldx(1, 2, 7, k), A.stx(1, 10, -16 + (k + 6) % 12, 2)]
    it += [A.ldx(1, 8, 7, 22), A.alu64("add", 8, 255), A.alu64("and", 8, 0xFF),
           A.ldx(2, 9, 7, 24), A.alu64("add", 9, 0x100), A.mov64_reg(2, 9), A.alu64("rsh", 2, 16), A.alu64("and", 9, 0xFFFF),
           A.alu64("add", 9, 2, reg=True), A.mov64_reg(2, 9), A.alu64("rsh", 2, 8), A.stx(1, 10, -20, 2), A.stx(1, 10, -19, 9),
           A.stx(1, 10, -18, 8)]
    for k in range(12):
        it += [A.ldx(1, 2, 10, -16 + k), A.stx(1, 7, k, 2)]
    for at, src in ((24, -20), (25, -19), (22, -18)):
        it += [A.ldx(1, 2, 10, src), A.stx(1, 7, at, 2)]
    it += [A.mov64_reg(0, 8), A.exit_(), "out", A.mov64_imm(0, 0), A.exit_()]
    return A.assemble(it)


def child(args) -> int:
    import numpy as np
    import torch

    import mimic_amd as M
    from mimic_amd import workloads as W

    dev = "cuda:0"
    buf, off, lens = W.make_skb_packets(args.packets, **W.IMIX)
    raw, rel = direct_program()
    runs = [("direct", ("skb_rewrite_direct", raw, rel), {})]
    if not args.direct_only:
        assert raw == W.prog_skb_rewrite_direct().raw, "the probe's copy of the direct program is stale"
        h = W.prog_skb_rewrite()
        runs += [("helper", (h.name, h.raw, h.relocs), {}), ("helper_knob_off", (h.name, h.raw, h.relocs), {"MIMIC_JIT_SKBSTORE": "0"})]
    if args.only:                                         # one run alone: the child a kernel trace is taken of
        runs = [r for r in runs if r[0] == args.only]
    vms, first = [], {}
    for name, p, env in runs:
        os.environ.update(env)                            # the knob is read when the kernel is generated
        vm = M.NewVM(M.VMOptEmulator(M.NewLinuxEmulator()), M.VMOptSetvCPUs(1 << 17), M.VMOptDevice(0))
        pid = vm.AddProgram(M.ProgramSpec(p[0], p[1], list(p[2])))
        batch = M.SKBBatch.from_numpy(buf, off, lens, device=dev, ifindex=1, schedule=M.SCHED_INTERLEAVED)
        res = M.XDPResults.empty(args.packets, dev, full=False)
        vm.RunSKBBatch(pid, batch, res)                   # builds the kernel; the first batch's result
        vm.SKBRelease()
        first[name] = (batch.pkt_data.cpu().numpy().copy(), res.r0[:args.packets].cpu().numpy().copy(), vm.LastExec())
        for k in env:
            del os.environ[k]
        vms.append((name, vm, pid, batch, res))
    ref = first[runs[0][0]]
    for name, (_, _, ex) in first.items():
        if ex != "jit":
            print(json.dumps({"error": f"{name}: ran on {ex}, not on the JIT"}))
            return 1
    for name, (pkt, r0, ex) in first.items():
        if not (np.array_equal(pkt, ref[0]) and np.array_equal(r0, ref[1])):
            print(json.dumps({"error": f"{name}: first batch differs from direct"}))
            return 1
    o = np.asarray(off).astype(np.int64) + 32       # frames the programs rewrite: IPv4, at least 34 bytes
    frames = int(((np.asarray(lens) >= 34) & (buf[o + 12] == 8) & (buf[o + 13] == 0)).sum())
    stream = torch.cuda.Stream(dev)                       # (the null stream would send the launches to the VM's own)
    out = {name: [] for name, *_ in vms}
    host = {name: [] for name, *_ in vms}
    for _ in range(args.inner):
        for name, vm, pid, batch, res in vms:

            def step():
                vm.RunSKBBatch(pid, batch, res, stream=stream, sync=False)
                vm.SKBRelease()

            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            for _ in range(args.steps):
                step()
            t1 = time.perf_counter()
            e1.record(stream)
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / args.steps)
            host[name].append((t1 - t0) * 1e3 / args.steps)   # the enqueue alone: a device time near it is host-bound
    print(json.dumps({"lib": os.environ.get("MIMIC_LIB", "libmimic_amd.so"), "exec": {n: first[n][2] for n in first},
                      "rewritten_frames": frames, "ms_per_batch": out, "host_enqueue_ms_per_batch": host}))
    for _, vm, *_ in vms:
        vm.close()
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2, help="at least 1")
    ap.add_argument("--inner", type=int, default=3, help="alternations inside a child")
    ap.add_argument("--parent", default="libmimic_parent.so")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--direct-only", action="store_true")
    ap.add_argument("--only", default="", help="with --child: this run alone (direct, helper or helper_knob_off)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.rounds < 1:
        ap.error("--rounds must be at least 1")
    base = [sys.executable, os.path.abspath(__file__), "--child", "--packets", str(args.packets), "--steps", str(args.steps),
            "--warmup", str(args.warmup), "--inner", str(args.inner)]
    have_parent = os.path.exists(os.path.join(ROOT, "mimic_amd", os.path.basename(args.parent)))
    samples = {"direct@parent": [], "direct": [], "helper": [], "helper_knob_off": []}
    enqueue = {k: [] for k in samples}
    execs = {}
    for _ in range(args.rounds):
        for lib in ([args.parent] if have_parent else []) + [None]:
            env = dict(os.environ)
            env.pop("MIMIC_LIB", None)
            if lib:
                env["MIMIC_LIB"] = os.path.basename(lib)
            r = subprocess.run(base + (["--direct-only"] if lib else []), env=env, capture_output=True, text=True, timeout=900)
            if r.returncode:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
                return r.returncode      # a failed child ends the probe: nothing more is started on the GPU
            doc = json.loads(r.stdout.strip().splitlines()[-1])
            for name, ms in doc["ms_per_batch"].items():
                samples[name + "@parent" if lib else name] += ms
                enqueue[name + "@parent" if lib else name] += doc["host_enqueue_ms_per_batch"][name]
            execs.update({(k + "@parent" if lib else k): v for k, v in doc["exec"].items()})
            frames = doc["rewritten_frames"]
    med = {k: statistics.median(v) for k, v in samples.items() if v}
    doc = {"packets": args.packets, "steps": args.steps, "warmup": args.warmup, "rewritten_frames": frames, "exec": execs,
           "ms_per_batch_median": med,
           "host_enqueue_ms_per_batch_median": {k: statistics.median(v) for k, v in enqueue.items() if v}, "ms_per_batch_samples": {k: v for k, v in samples.items() if v},
           "ratio_helper_over_baseline": med["helper"] / med.get("direct@parent", med["direct"]),
           "ratio_helper_over_knob_off": med["helper"] / med["helper_knob_off"],
           "baseline": "direct@parent" if "direct@parent" in med else "direct"}
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
