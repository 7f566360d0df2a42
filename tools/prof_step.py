"""Which ATen ops (copies, fills, zeros, cat / stack, adds) does a steady-state eager train step still issue, and from where?
torch.profiler (with stacks) over a few warm steps of bench.py's default step, per step, grouped by op, first project frame above it
("?" = issued by the autograd engine, no Python frame) and input shapes - the train-step counterpart of tools/prof_synth.py.  Set-up
launches (parameter upload, batch) are excluded by construction: only warm steps are profiled.  The library's own kernels, casts and
adds included, are counted by the rocprofv3 kernel trace (tools/rocpd_summary.py).
usage: python tools/prof_step.py [bench.py flags, e.g. --frame-level]"""
import collections
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

STEPS = 4


def main():
    args = bench.parse(sys.argv[1:])
    dev = torch.device("cuda:0")
    model, loss_fn, opt, b, _, _ = bench.build(args, dev, 0, 1)
    step, _ = bench.make_step(model, loss_fn, opt, b, None)
    for _ in range(6):
        step()
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU], with_stack=True, record_shapes=True) as prof:
        for _ in range(STEPS):
            step()
        torch.cuda.synchronize()
    evs = list(prof.events())
    print("== ATen ops with a project frame (CPU side), per step")
    ops_ = collections.Counter()
    for e in evs:
        if e.name.startswith("aten::") and e.name in ("aten::copy_", "aten::zero_", "aten::fill_", "aten::cat", "aten::stack", "aten::clone",
                                                       "aten::_to_copy", "aten::contiguous", "aten::add", "aten::mul", "aten::ones_like",
                                                       "aten::zeros", "aten::zeros_like", "aten::sum", "aten::add_"):
            st = [f for f in (e.stack or []) if "fastspeech2_amd" in f or "bench.py" in f]
            ops_[(e.name, (st[0] if st else "? (autograd engine / no Python frame)")[-90:], str(e.input_shapes)[:40])] += 1
    for (n, st, shp), c in sorted(ops_.items(), key=lambda kv: -kv[1])[:50]:
        print(f"{c / STEPS:6.2f}  {n:20s} {st:90s} {shp}")


if __name__ == "__main__":
    main()
