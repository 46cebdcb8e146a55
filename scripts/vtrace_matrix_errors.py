#!/usr/bin/env python3
"""Worst observed error of every V-trace kernel variant in every input regime of
tests/test_gpu_vtrace_matrix.py (section f), against the fp64 reference tests/vtrace_cases.ref_numpy.

Per regime and variant (1 = LDS kernel, 2 = column kernel, 3 = sequence kernel, 4 = streaming
kernel), the worst over the regime's shapes of
  unit:  |d| / max(1, |ref|), the project's 1e-5 bar's own measure, per output;
  bars:  the same error in units of the bar the test applies (1e-5, times the derived scale of
         the wide regimes: the test's module docstring), per output.
A measurement, no threshold: the test asserts. Prints one JSON line and writes it to
profiles/vtrace_matrix_errors.json.

    python scripts/vtrace_matrix_errors.py [--out profiles/vtrace_matrix_errors.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vtrace_cases as vc  # noqa: E402

KEYS = ("vs", "pg_adv", "dlogits", "dvalue", "losses")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vtrace_matrix_errors.json"))
    args = ap.parse_args()
    res = {}
    for regime in vc.UNIT_REGIMES + vc.WIDE_REGIMES:
        wide = regime in vc.WIDE_REGIMES
        res[regime] = {"bar": "1e-5 * derived scale" if wide else "1e-5"}
        for variant in (1, 2, 3, 4):
            unit = dict.fromkeys(KEYS, 0.0)
            bars = dict.fromkeys(KEYS, 0.0)
            for case in vc.cases_f((regime,)):
                *inp, hp = vc.build(*case)
                ref = vc.ref_numpy(*inp, **hp)
                out = vc.run_vtrace(*inp, variant=variant, guard=True, **hp)
                ones = {k: 1.0 for k in KEYS}
                u = vc.scaled_errors(out, ref, ones)
                b = vc.scaled_errors(out, ref, vc.wide_scales(inp[0], inp[1], ref)) if wide else u
                for k in KEYS:
                    unit[k] = max(unit[k], u[k] * vc.TOL)
                    bars[k] = max(bars[k], b[k])
            res[regime][f"variant_{variant}"] = {
                "unit": {k: float(f"{v:.3e}") for k, v in unit.items()},
                "bars": {k: float(f"{v:.3e}") for k, v in bars.items()},
                "worst_bars": float(f"{max(bars.values()):.3e}")}
    doc = {"what": "worst observed error of the V-trace kernels per input regime and variant against "
                   "the fp64 numpy reference; shapes (T, B, A) = " + str(list(vc.EF_SHAPES)) +
                   "; a measurement, the test asserts",
           "shapes": [list(s) for s in vc.EF_SHAPES], "regimes": res}
    line = json.dumps(doc)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
