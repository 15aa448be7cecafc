"""The environment knobs the native code reads and DESIGN.md's table of them (3.2.1) are the same
set: a knob added or retired in mimic_amd/csrc/ without its row, or the other way round, fails here."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _code_knobs():
    """MIMIC_* names passed to getenv, directly or through jit.cpp's off() / on() / num()."""
    names = set()
    for path in glob.glob(os.path.join(ROOT, "mimic_amd", "csrc", "*")):
        if path.endswith(".inc"):   # generated: the headers again
            continue
        with open(path, errors="replace") as f:
            names.update(re.findall(r'\b(?:getenv|off|on|num)\(\s*"(MIMIC_[A-Z0-9_]+)"', f.read()))
    return names


def _table_knobs():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    sec = text.split("### 3.2.1 Environment knobs", 1)[1].split("\n### ", 1)[0]
    return set(re.findall(r"^\| `(MIMIC_[A-Z0-9_]+)` \|", sec, re.M))


def test_design_lists_every_knob_the_code_reads():
    code, table = _code_knobs(), _table_knobs()
    assert len(code) > 20
    assert code == table, f"only in csrc: {sorted(code - table)}; only in DESIGN.md 3.2.1: {sorted(table - code)}"
