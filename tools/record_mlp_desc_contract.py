#!/usr/bin/env python3
"""Record tests/golden/mlp_desc_contract.json, the fixture of tests/test_mlp_desc_contract.py.

    python tools/record_mlp_desc_contract.py --lib PATH/libhgnn_hip.so [--reword 'CASE_GLOB=NEW TEXT' ...]

PATH is the library of the commit whose behaviour is being frozen -- the one BEFORE the change under test, never the
code under test.  Host code only (no GPU): the case lists are the test module's own.

--reword: the recorded hgnn_last_error() text of the refusal cases matching CASE_GLOB (``entry/case id``, fnmatch) is
replaced by NEW TEXT -- for a message that is reworded ON PURPOSE by the change under test; the return code is kept as
recorded.  Every rewording is written into the fixture next to the recorded text it replaces.
"""
import argparse
import ctypes
import fnmatch
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_mlp_desc_contract as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", required=True)
    ap.add_argument("--reword", action="append", default=[], metavar="CASE_GLOB=NEW TEXT")
    args = ap.parse_args()
    lib = T.bind(ctypes.CDLL(os.path.abspath(args.lib)))
    cases = T.verdict_cases()
    refusals = T.refusals(lib)
    reworded = {}
    for item in args.reword:
        glob, text = item.split("=", 1)
        hits = [k for k in refusals if fnmatch.fnmatch(k, glob)]
        if not hits:
            sys.exit(f"--reword {glob!r} matches no case")
        for k in hits:
            reworded[k] = {"recorded": refusals[k][1], "reworded": text}
            refusals[k][1] = text
    fixture = {"entries": list(T.ENTRIES), "cases_sha256": T.cases_hash(cases), "verdicts": T.verdicts(lib, cases),
               "refusals": refusals, "reworded": reworded}
    with open(T.FIXTURE, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{T.FIXTURE}: {len(cases)} verdict cases, {len(refusals)} refusal cases, {len(reworded)} reworded")


if __name__ == "__main__":
    main()
