#!/usr/bin/env python3
"""Generate tests/golden/ref_live_cases.npz FROM THE REFERENCE ITSELF: the levels of the three clouds of
tests/test_oracle_vs_ref.py, computed by the reference's own compiled HEM extension (oracle/_ref, `make -C oracle ref`)
through oracle/run_ref.py, one fresh process per case.  Data only: the reference's outputs and a fingerprint of each input.

    python tests/golden/make_golden_ref_live.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_oracle_vs_ref as T  # noqa: E402


def main():
    if not T.REF:
        raise SystemExit("oracle/_ref is not built: run `make -C oracle ref` where the reference sources are")
    out = {"numpy_version": np.array(np.__version__)}
    for n, h, deg, levels, params in T.CASES:
        c = T._cloud(n, h, deg)
        ref = T._run_ref(c, levels, **params)
        out[f"n{n}_input_sum"] = np.float64(T._input_sum(c))
        for k in range(levels):
            for f in T.FIELDS:
                out[f"n{n}_{f}_{k}"] = ref[f"{f}_{k}"]
        print(n, "levels:", [int(ref[f"xyz_{k}"].shape[0]) for k in range(levels)])
    np.savez_compressed(T.STORED, **out)
    print("wrote", T.STORED, os.path.getsize(T.STORED), "bytes")


if __name__ == "__main__":
    main()
