"""Fingerprints of the JIT kernels' machine code, on a CPU host (hipRTC needs no GPU).

    python tools/jit_fingerprint.py OUT.json

For every kernel the GPU suite compiles (the jit_kernels() of each tests/test_gpu_*.py module, what
the session prewarm collects) and every bench kernel, OUT.json records the sha256 and size of the
gfx950 code object's .text section and its jit.kernel_resources.  Two libraries (MIMIC_LIB selects
one) whose files are equal generate the same machine code for all of them: a refactor of the
generator or of the device runtime headers can be shown to change no kernel without a GPU.  Whole
code objects are not compared: their other sections change with a comment in the source."""
import glob
import hashlib
import importlib
import json
import os
import struct
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from mimic_amd import _lib, jit as J, workloads as W  # noqa: E402


def text_section(elf: bytes) -> bytes:
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    sec = [struct.unpack_from("<IIQQQQ", elf, shoff + i * shentsize) for i in range(shnum)]   # name, type, flags, addr, off, size
    names = elf[sec[shstrndx][4]:sec[shstrndx][4] + sec[shstrndx][5]]
    for name, _, _, _, off, size in sec:
        if names[name:names.index(b"\0", name)] == b".text":
            return elf[off:off + size]
    raise KeyError(".text")


def sources():
    """{label: kernel source}: the GPU suite's kernels, then the bench configs'."""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py"))):
        name = os.path.basename(path)[:-3]
        fn = getattr(importlib.import_module(name), "jit_kernels", None)
        for n, k in enumerate(fn() if fn else []):
            out[f"{name}[{n}]"] = J.kernel_source(list(k[0]), *k[1:])
    cls, p5, ft = W.prog_classifier(), W.prog_parse5(), W.prog_flowtrack()
    skb = [p.raw for p in W.skb_programs()[0]]
    progs = [(cls.raw, cls.relocs)]
    out["bench:classifier"] = J.kernel_source([cls.raw], _lib.CTX_XDP, J.vc_slots(progs, cls.maps))
    out["bench:parse5"] = J.kernel_source([p5.raw], _lib.CTX_XDP, J.vc_slots([(p5.raw, p5.relocs)], p5.maps))
    out["bench:flowtrack"] = J.kernel_source([ft.raw], _lib.CTX_XDP, J.vc_slots([(ft.raw, ft.relocs)], ft.maps))
    out["bench:flowtrack:no_early_loads"] = J.kernel_source([ft.raw], _lib.CTX_XDP, J.vc_slots([(ft.raw, ft.relocs)], ft.maps),
                                                           no_early_loads=True)
    out["bench:skb"] = J.kernel_source(skb, _lib.CTX_SKB)
    for own in (False, True):   # the default line's VM: 1M packets on 256K vCPUs
        out["bench:classifier:" + ("own" if own else "spread")] = J.kernel_source(
            [cls.raw], _lib.CTX_XDP, (), J.spread_spec(progs, cls.maps, 1 << 18, own=own))
    out["bench:classifier:proc"] = J.kernel_source([cls.raw], _lib.CTX_XDP, proc=True)
    return out


def fingerprint(src: str) -> dict:
    code = J.code_object(src)
    text = text_section(code)
    return {"text_sha256": hashlib.sha256(text).hexdigest(), "text_bytes": len(text), "resources": J.kernel_resources(code)}


if __name__ == "__main__":
    srcs = sources()
    distinct = sorted(set(srcs.values()))
    # a cache of this run's own: every kernel is compiled by the library under test, in jit.py's
    # parallel workers (which survive a worker that dies), and read back from there
    with tempfile.TemporaryDirectory(prefix="mimic_fp_") as cache:
        os.environ["MIMIC_JIT_CACHE"] = cache
        print(J._compile_parallel(distinct, 0))
        done = {s: fingerprint(s) for s in distinct}
    with open(sys.argv[1], "w") as f:
        json.dump({label: done[s] for label, s in srcs.items()}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(srcs)} kernels ({len(distinct)} distinct sources) -> {sys.argv[1]}")
