"""Derives the bars of tests/test_melgan_gpu.py on the CPU, from the number formats alone (never from the code under test; the
method of make_bf16_bars.py).  For every end-to-end shape (B, T) of tests/melgan_ref.py and every probed stage, as relative Frobenius
distances to the fp64 restatement:

  fp32: d32 = the restatement run in torch-CPU float32 against float64, on the test's own weights and input (seed 0).
        bar = 4 x d32: the kernels sum in another order than torch's CPU convolutions.
  bf16: dbf = the restatement with the bf16 product's storage points emulated (melgan_ref.emulate_bf16: bf16 weight images, every
        stored activation rounded) against the exact one, over seeds 0..7.  bar = 2 x max over the seeds.

    python tests/golden/make_melgan_bars.py        # ~1 min, writes tests/golden/melgan_bars.json
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import melgan_ref as R  # noqa: E402

N_SEEDS = 8
F32_FACTOR, BF16_FACTOR = 4.0, 2.0


def main():
    table = {"f32_factor": F32_FACTOR, "bf16_factor": BF16_FACTOR, "n_seeds": N_SEEDS, "metric": "relative Frobenius distance to fp64",
             "shapes": {}}
    for B, T in R.SHAPES:
        d32, dbf = None, {s: [] for s in R.STAGES}
        for seed in range(N_SEEDS):
            sd, x = R.make_case(seed, B, T)
            w64 = R.plain_weights(sd)
            with torch.no_grad():
                exact = R.forward(w64, x.double())
                if seed == 0:
                    o32 = R.forward(R.plain_weights(sd, torch.float32), x)
                    d32 = {s: R.rel(o32[s], exact[s]) for s in R.STAGES}
                emu = R.emulate_bf16(w64, x.double())
            for s in R.STAGES:
                dbf[s].append(R.rel(emu[s], exact[s]))
        table["shapes"][f"{B}x{T}"] = {
            "fp32": {s: {"d32": d32[s], "bar": F32_FACTOR * d32[s]} for s in R.STAGES},
            "bf16": {s: {"emulated": dbf[s], "bar": BF16_FACTOR * max(dbf[s])} for s in R.STAGES}}
        print(B, T, {s: f"{table['shapes'][f'{B}x{T}']['fp32'][s]['bar']:.2e}/{table['shapes'][f'{B}x{T}']['bf16'][s]['bar']:.2e}" for s in R.STAGES},
              flush=True)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "melgan_bars.json"), "w") as f:
        json.dump(table, f, indent=1)


if __name__ == "__main__":
    main()
