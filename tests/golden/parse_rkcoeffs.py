"""Reads the Runge-Kutta tableau of the reference's re-integrator out of its own header at fixture-generation time.

    python tests/golden/parse_rkcoeffs.py        # writes tests/golden/rk_tables.json

Runs in the build container only (the reference does not travel); what is committed is data: the four numeric tables of
RKCoeffs<RKOptions::DOPRI87> in /root/reference/src/Integrators/RKCoeffs.h -- ACoeffs -> "a" [12][12], Times -> "c" [12], BCoeffs -> "b" [13]
(the propagated order-8 weights), CCoeffs -> "bhat" [13] (the order-7 weights of the estimate) -- each constexpr initialiser evaluated
in IEEE double exactly as the C++ compiler folds it (quotients of literals; an integer literal beside a floating one converts
exactly).  tests/test_integ_cpu.py compares csrc/rk_tables.h against this file bit for bit, and tests/integ_checker.py takes its
tableau from it.  The precedent is parse_lglcoeffs.py.
"""
from __future__ import annotations

import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = "/root/reference/src/Integrators/RKCoeffs.h"
NAMES = {"ACoeffs": "a", "Times": "c", "BCoeffs": "b", "CCoeffs": "bhat"}


def _strip_comments(text: str) -> str:
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def parse(path: str = HEADER):
    text = _strip_comments(open(path).read())
    pos = re.search(r"struct\s+RKCoeffs<\s*RKOptions::DOPRI87\s*>\s*\{", text).start()
    block = text[pos:]
    out = {}
    for m in re.finditer(r"static\s+constexpr\s+([^=;]+?)\s+(\w+)\s*=\s*(.*?);", block, flags=re.S):
        typ, name, init = m.group(1).strip(), m.group(2), m.group(3).strip()
        if name not in NAMES or "STDarray" not in typ:
            continue
        body = re.sub(r"STDarray\s*<[^{}]*?>\s*(?=\{)", "", init)
        body = re.sub(r",\s*\}", "}", body)                                   # (trailing commas)
        body = re.sub(r"(?<![\w.])(\d+)(?![\w.])", r"\1.0", body)               # integer literals: the quotient is a double one
        val = eval(body.replace("{", "[").replace("}", "]"), {"__builtins__": {}}, {})   # noqa: S307 -- arithmetic on literals
        out[NAMES[name]] = val
    assert sorted(out) == ["a", "b", "bhat", "c"], sorted(out)
    assert len(out["a"]) == 12 and all(len(r) == 12 for r in out["a"]) and len(out["c"]) == 12
    assert len(out["b"]) == 13 and len(out["bhat"]) == 13
    return out


def main():
    if not os.path.exists(HEADER):
        sys.exit(f"{HEADER} not found: this script runs in the build container only")
    tabs = parse()
    path = os.path.join(HERE, "rk_tables.json")
    with open(path, "w") as f:
        json.dump({"source": "src/Integrators/RKCoeffs.h (reference), RKCoeffs<DOPRI87>, parsed by tests/golden/parse_rkcoeffs.py",
                   "stages": 13, "tables": tabs}, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
