"""Writes tests/golden/icp_acc_tolerance.json: per (scene, kind) of tests/icp_acc_model.py, what float64 costs the model itself --
max over the slots and the losses of |acc64 - acc_hp| / (sum |term| + tiny), acc_hp the same model in 50-digit arithmetic (mpmath) on
the first 300 matched pairs of the scene.  Kinds 0 and 4 are 0 by definition.  tests/test_icp_acc_cpu.py recomputes the file.

    python tests/golden/make_golden_icp_acc.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import icp_acc_model as A  # noqa: E402

if __name__ == "__main__":
    tol = A.tolerances()
    with open(A.TOLERANCE_JSON, "w") as fh:
        json.dump(tol, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for k in sorted(tol):
        print(f"{k}: {tol[k]:.3e}")
