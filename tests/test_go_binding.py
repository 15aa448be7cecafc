"""The Go binding keeps mimic's own surface (go/: gpu.go, gpu_stub.go, mimic_gpu.patch).  No Go
toolchain exists in this image, so the binding is checked structurally:

* the patch to vm.go / emulator_linux_.go only ADDS lines, none of them a top-level declaration, so
  every exported func keeps its signature (NewVM, AddProgram, NewProcess, SetCPUID, Step, Run,
  Cleanup) and every struct field is still there, the added fields after them;
* the hooks the patch adds call methods that gpu.go (engine build) and gpu_stub.go (default build)
  both define with the same parameters;
* every C function gpu.go calls is declared in include/mimic_amd.h with that many parameters, and
  every C struct field it sets exists there; the context fields it reads exist in
  LinuxContextXDP / LinuxContextSKBuff / SK / FlowKeys / NetDev as mimic_amd mirrors them.
Everything is read from this repository: the patch carries the lines it hooks under as context."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "go")
HDR = os.path.join(ROOT, "include", "mimic_amd.h")


def _read(p):
    with open(p) as f:
        return f.read()


def _strip_comments(src):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def _hunks(patch, name):
    """The hunks of the patch's file `name`: lists of (tag, text) with tag ' ' (context) or '+'."""
    body = patch.split("+++ b/" + name + "\n", 1)[1].split("\n--- a/", 1)[0]
    out = []
    for h in re.split(r"^@@[^\n]*\n", body, flags=re.M)[1:]:
        out.append([(l[:1], l[1:]) for l in h.split("\n") if l[:1] in (" ", "+")])
    return out


def _added(hunks):
    return [t for h in hunks for tag, t in h if tag == "+"]


def test_patch_only_adds_lines():
    patch = _read(os.path.join(GO, "mimic_gpu.patch"))
    files = re.findall(r"^\+\+\+ b/(\S+)", patch, flags=re.M)
    assert files == ["vm.go", "emulator_linux_.go"]
    removed = [l for l in patch.splitlines() if l.startswith("-") and not l.startswith("---")]
    assert removed == [], removed


def test_patched_vm_keeps_the_reference_signatures():
    """The patch removes and rewrites nothing (test_patch_only_adds_lines), so every declaration of
    the package it applies to stays as it is; what it adds declares no func, type, const or var at
    top level, so the exported surface of vm.go / emulator_linux_.go is unchanged.  The hooks sit
    directly under the signatures the drop-in names, which the patch carries as context."""
    patch = _read(os.path.join(GO, "mimic_gpu.patch"))
    for f in ("vm.go", "emulator_linux_.go"):
        for l in _added(_hunks(patch, f)):
            assert l == "" or l.startswith("\t"), (f, l)   # nothing added at top level
    want = {
        "step": "func (p *Process) Step() (exited bool, err error) {",
        "run": "func (p *Process) Run(ctx context.Context) error {",
        "free": "func (p *Process) Cleanup() error {",
    }
    hunks = _hunks(patch, "vm.go")
    for hook, sig in want.items():
        hs = [h for h in hunks if any(tag == "+" and f"p.gpu.{hook}(" in t for tag, t in h)]
        assert len(hs) == 1, hook
        h = hs[0]
        first = next(i for i, (tag, _) in enumerate(h) if tag == "+")
        assert h[first - 1] == (" ", sig), (hook, h[first - 1])
        assert h[first] == ("+", "\tif p.gpu != nil {")


def _added_fields(hunk):
    """Names of the struct fields a hunk adds directly above the struct's closing brace."""
    idx = [i for i, (tag, _) in enumerate(hunk) if tag == "+"]
    if not idx or hunk[idx[-1] + 1:idx[-1] + 2] != [(" ", "}")]:
        return None
    assert idx == list(range(idx[0], idx[-1] + 1))   # one block
    code = [_strip_comments(t).strip() for _, t in hunk[idx[0]:idx[-1] + 1]]
    return [c.split()[0] for c in code if c]


def test_patched_structs_keep_every_reference_field():
    """The fields the patch adds to VMSettings, VM and Process come after every field the struct
    already has: each is added directly above the struct's closing brace, below the struct's last
    own field (a context line of the hunk).  VMSettings ends with GPU."""
    hunks = _hunks(_read(os.path.join(GO, "mimic_gpu.patch")), "vm.go")
    last_own = {"VirtualCPUs": ["GPU"], "processPool": ["gpu"], "exited": ["gpu"]}
    seen = {}
    for h in hunks:
        first = next(i for i, (tag, _) in enumerate(h) if tag == "+")
        above = [t for tag, t in h[:first] if tag == " " and _strip_comments(t).strip()]
        key = above[-1].split()[0] if above else ""
        if key in last_own and re.match(r"\t\w+\s+\S+$", _strip_comments(above[-1]).rstrip()):
            seen[key] = _added_fields(h)
    assert seen == last_own, seen


def _methods(src):
    """(receiver type, name) -> normalised parameter list of the gpu* helpers."""
    out = {}
    for m in re.finditer(r"^func (?:\(\w+ \*?(\w+)\) )?(\w+)\(([^)]*)\)", _strip_comments(src), flags=re.M):
        params = re.sub(r"\s+", " ", m.group(3)).strip()
        out[(m.group(1) or "", m.group(2))] = params
    return out


def test_engine_and_stub_builds_define_the_same_hooks():
    eng = _methods(_read(os.path.join(GO, "gpu.go")))
    stub = _methods(_read(os.path.join(GO, "gpu_stub.go")))
    patch = _read(os.path.join(GO, "mimic_gpu.patch"))
    called = set(re.findall(r"\.gpu\.(\w+)\(", patch)) | set(re.findall(r"\b(newGPUVM)\(", patch))
    assert called == {"newGPUVM", "capture", "addProgram", "newProcess", "setCPU", "step", "run", "free", "addMap"}
    for name in called:
        ek = [k for k in eng if k[1] == name]
        sk = [k for k in stub if k[1] == name]
        assert len(ek) == 1 and len(sk) == 1, name
        assert ek[0] == sk[0] and eng[ek[0]] == stub[sk[0]], (name, eng[ek[0]], stub[sk[0]])
    for k in (("", "VMOptGPU"), ("VM", "RunBatch")):
        assert eng[k] == stub[k], k
    for f in ("gpu.go", "gpu_stub.go"):
        s = _strip_comments(_read(os.path.join(GO, f)))
        s = re.sub(r'"(?:\\.|[^"\\])*"', '""', s)
        assert s.count("{") == s.count("}") and s.count("(") == s.count(")"), f


def _c_protos():
    hdr = _strip_comments(_read(HDR))
    protos = {}
    for m in re.finditer(r"\b(?:int|void|long|const char \*)\s*(mimic_\w+)\(([^;]*?)\);", hdr, flags=re.S):
        args = m.group(2).strip()
        protos[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return protos


def _call_args(src, start):
    depth, i, n, seen = 0, start, 0, False
    while True:
        c = src[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                return n + (1 if seen else 0)
        elif c == "," and depth == 1:
            n += 1
        elif not c.isspace() and depth >= 1:
            seen = True
        i += 1


def test_cgo_calls_match_the_header():
    src = _strip_comments(_read(os.path.join(GO, "gpu.go")))
    protos = _c_protos()
    calls = list(re.finditer(r"\bC\.(mimic_\w+)\(", src))
    assert len(calls) > 20
    for m in calls:
        name = m.group(1)
        assert name in protos, name
        assert _call_args(src, m.end() - 1) == protos[name], name
    hdr = _read(HDR)
    for m in re.finditer(r"C\.(mimic_\w+)\{(.*?)\}\s*$", src, flags=re.S | re.M):
        td = re.search(r"typedef struct \{(.*?)\}\s*" + m.group(1) + ";", hdr, flags=re.S)
        assert td, m.group(1)
        for fld in re.findall(r"(\w+):", m.group(2)):
            fld = "type" if fld == "_type" else fld
            assert re.search(r"\b" + fld + r"\b", td.group(1)), (m.group(1), fld)


def test_context_fields_exist_in_the_reference():
    """Every exported context field gpu.go reads is a field of the same struct in the package's API
    as mimic_amd mirrors it (vm.py's LinuxContextXDP / LinuxContextSKBuff / SK / FlowKeys / NetDev
    dataclasses, each citing the Go declaration it restates)."""
    import dataclasses

    import mimic_amd as M

    src = _strip_comments(_read(os.path.join(GO, "gpu.go")))
    fields = {n: [f.name for f in dataclasses.fields(getattr(M, n))]
              for n in ("LinuxContextXDP", "LinuxContextSKBuff", "SK", "FlowKeys", "NetDev")}
    for f in ("Headroom", "Tailroom", "Packet", "IngessIfIndex", "RxQueueIndex", "EgressIfIndex"):
        assert f in fields["LinuxContextXDP"] and f"c.{f}" in src, f
    for f in ("Packet", "SK", "Dev", "FlowKeys"):
        assert f in fields["LinuxContextSKBuff"], f
    read = re.findall(r"\bsk\.(\w+)", src)
    assert len(read) >= 14
    for f in read:
        # the unexported address fields (srcIP4 ...) are the ones SK's UnmarshalJSON fills from the
        # exported strings of the same name
        assert (f if f[0].isupper() else f[0].upper() + f[1:]) in fields["SK"], f
    for f in re.findall(r"\bfk\.(\w+)", src):
        assert f in fields["FlowKeys"], f
    assert "IFIndex" in fields["NetDev"]
