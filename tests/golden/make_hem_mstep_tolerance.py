"""Writes tests/golden/hem_mstep_tolerance.json: per case of tests/hem_mstep_model.py and output field, K_ref = the largest
|oracle - model| / (2^-24 mag) over the elements of the level and the SH widths of the case -- what the reference's float32 arithmetic
in serial order (the CPU oracle) costs against the float64 model, in units of one float32 rounding of the element's magnitude.  Only
the model and the oracle produce these numbers; no kernel runs.  tests/test_hem_mstep_cpu.py recomputes the file.

    python tests/golden/make_hem_mstep_tolerance.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hem_mstep_model as M  # noqa: E402
from oracle import oracle as O  # noqa: E402

if __name__ == "__main__":
    tol = M.tolerances(O)
    with open(M.TOLERANCE_JSON, "w") as fh:
        json.dump(tol, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for name in M.CASES:
        print(name, " ".join(f"{f} {tol[name][f]:.2f}" for f in M.FIELDS))
