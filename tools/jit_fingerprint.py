"""Fingerprints of the JIT kernels, on a CPU host (neither mode needs a GPU).

    python tools/jit_fingerprint.py OUT.json            machine code
    python tools/jit_fingerprint.py --source OUT.json   source text, under every knob setting

Machine code.  For every kernel the GPU suite compiles (the jit_kernels() of each
tests/test_gpu_*.py module, what the session prewarm collects) and every bench kernel, OUT.json
records the sha256 and size of the gfx950 code object's .text section and its jit.kernel_resources.  Two libraries (MIMIC_LIB selects
one) whose files are equal generate the same machine code for all of them: a refactor of the
generator or of the device runtime headers can be shown to change no kernel without a GPU.  Whole
code objects are not compared: their other sections change with a comment in the source.  This is
the mode for a change that may alter the generated text (a comment, an alias, indentation) or a
runtime header, and must leave the code as it was.

Source.  No compile: for every label of sources(), under each setting of KNOBS and SUITE_KNOBS (one child process
per setting, its environment cleared of every other MIMIC_JIT_ variable), OUT.json records the
sha256 and byte length of the source text; the file's own sha256 is printed.  The source text
is the code-object cache key, so two libraries whose files are equal generate the same kernels,
cache entries and speed under every knob: this is the mode for a refactor of the generator (jit.cpp)
that touches no runtime header, and it proves nothing about a change to one (the headers are
included by the text, not part of it)."""
import glob
import hashlib
import importlib
import json
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from mimic_amd import _lib, jit as J, workloads as W  # noqa: E402


# the knob matrix of the source mode: "" is the default, every other name carries the MIMIC_JIT_ prefix
KNOBS = ("", "FAST=0", "PREFETCH=0", "XPF=1", "LPF=1", "NTRES=0", "CENSUS=1", "CTXCHECK=1", "COLD=call", "COLD=inline",
         "COLD=defer", "DISPATCH=0", "RETDISPATCH=1", "VC=0", "LDSSTK=0", "SKBLDS=0", "SMLDS=0", "SPEC=0", "COMBINE=0",
         "HCHUNK=0", "WAVES=2", "DEFS=A,B=2", "INC=0", "FWD=0", "ELIDE=0", "WINDOW=0", "HASH=0", "TAIL=0", "SKBFIELD=0")
# settings that change no bench kernel (tests/test_jit_cpu.py holds every KNOBS entry to changing one): the inline
# bpf_skb_store_bytes changes the kernels of tests/test_gpu_storematrix.py, which sources() lists
SUITE_KNOBS = ("SKBSTORE=0",)


def knob_env(setting: str) -> dict:
    """The environment variable a KNOBS entry sets ({} for the default)."""
    name, _, value = setting.partition("=")
    return {"MIMIC_JIT_" + name: value} if setting else {}


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
    out.update(bench_sources())
    return out


def bench_sources():
    """{label: kernel source} of the bench configs' kernels."""
    out = {}
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


def source_digests() -> dict:
    """{label: sha256 and length of its source} under this process's environment."""
    return {label: {"sha256": hashlib.sha256(s.encode()).hexdigest(), "bytes": len(s.encode())} for label, s in sources().items()}


def source_mode(out_path: str) -> None:
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MIMIC_JIT_")}
    doc = {}
    for setting in KNOBS + SUITE_KNOBS:   # a child each: MIMIC_JIT_CTXCHECK is read once per process
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--source-child"], env=dict(clean, **knob_env(setting)),
                             capture_output=True, text=True, check=True).stdout
        doc[setting or "default"] = json.loads(out.strip().splitlines()[-1])
    body = json.dumps(doc, indent=1, sort_keys=True) + "\n"
    with open(out_path, "w") as f:
        f.write(body)
    print(f"{len(doc['default'])} kernels x {len(doc)} settings -> {out_path}, sha256 {hashlib.sha256(body.encode()).hexdigest()}")


if __name__ == "__main__":
    if sys.argv[1] == "--source-child":
        print(json.dumps(source_digests()))
        sys.exit(0)
    if sys.argv[1] == "--source":
        source_mode(sys.argv[2])
        sys.exit(0)
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
