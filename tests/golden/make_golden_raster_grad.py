#!/usr/bin/env python3
"""Generate tests/golden/raster_grad_tolerance.json: per scene of ``tests/raster_grad_model.GPU_SCENES`` and per output array of the
backward pass (xyz, cov6, raw_opacity, dc, sh_rest), what float32 costs the NumPy model itself --
``max |g32 - g64| / (scale + tiny)``, the model run in float32 with the kernels' operation order against the model run in float64, ``scale``
the sum of the absolute values of the terms each entry is made of.  tests/test_raster_grad_gpu.py allows the kernel 4 x that figure;
tests/test_raster_grad_cpu.py checks that the file is what the model gives.  NumPy only, no GPU.

    python tests/golden/make_golden_raster_grad.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
import raster_grad_model as G  # noqa: E402


def main():
    out = {name: G.float32_cost(name) for name in G.GPU_SCENES}
    with open(os.path.join(HERE, "raster_grad_tolerance.json"), "w") as f:
        json.dump(out, f, indent=1)
    for name, row in out.items():
        print(name, row)


if __name__ == "__main__":
    main()
