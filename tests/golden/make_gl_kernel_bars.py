"""Writes tests/golden/gl_kernel_bars.json: for every elementwise case of tests/gl_cases.py, 4 x the largest distance between the
numpy oracle tests/gl_ref.py evaluated in float32 and in fp64, normalised as tests/test_griffin_lim_kernels_gpu.py normalises the
kernels' error (tests/gl_cases.measure).  4 x is the margin of tests/golden/griffin_lim.npz: room for a device cosf, sinf or atan2f
a few ulp wider than a correctly rounded one.  Runs on the CPU; nothing here touches the shared library.

    python tests/golden/make_gl_kernel_bars.py

tests/test_griffin_lim_cpu.py regenerates the numbers and requires them to equal the file."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import gl_cases as C                                             # noqa: E402


def main():
    out = C.measure()
    with open(C.BARS_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
