"""Ragged batches for the corpus front end (preprocess, prepare_align, align, pitch, resample, audio): how items are packed into
padded batches, how a batch's rows reach the device, and how `(x, lens)` is validated before a launch.  Plain Python: nothing here
needs the shared library.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

_PACKERS = ThreadPoolExecutor(max_workers=4)        # rows of a batch are packed side by side: numpy copies and fills without the GIL


# ------------------------------------------------------------------------------------------------ packing
def greedy_batches(dims, budget, cost):
    """Longest first, then greedy packing of PADDED batches.  `dims[i]` is the tuple of item i's padded extents, `cost(n, *maxima)`
    what a batch of n items padded to those per-extent maxima costs.  Items are taken in the order (-d0, -d1, ..., i); a batch is
    closed when the next item would take it over `budget`, and always holds at least one item.  Yields lists of indices."""
    batch, top = [], ()
    for i in sorted(range(len(dims)), key=lambda i: tuple(-d for d in dims[i]) + (i,)):
        grown = tuple(map(max, top, dims[i])) if batch else tuple(dims[i])
        if batch and cost(len(batch) + 1, *grown) > budget:
            yield batch
            batch, grown = [], tuple(dims[i])
        batch.append(i)
        top = grown
    if batch:
        yield batch


def padded_samples(n, N):
    """The `cost` of audio: n rows of N samples."""
    return n * N


def keyed_batches(keys, dims, budget, cost):
    """`greedy_batches` within each distinct key (a batch never mixes source rates: one filter per launch), keys ascending, under
    `budget(key)`.  Yields (key, indices)."""
    for k in sorted(set(keys)):
        idx = [i for i, v in enumerate(keys) if v == k]
        for batch in greedy_batches([dims[i] for i in idx], budget(k), cost):
            yield k, [idx[i] for i in batch]


# ------------------------------------------------------------------------------------------------ staging
class Staging:
    """One pinned float32 host buffer through which the rows of a ragged batch reach the device.  The rule it owns: `to` issues
    an asynchronous H2D copy, so the buffer must not be rewritten before that copy has read it; `to` records an event and the next
    `pack` waits for it.  Where the caller has blocked on a D2H copy of the batch's results in between, that wait is free."""

    def __init__(self):
        self._buf = self._view = self._copied = None

    def pack(self, rows, clip=False):
        """[1-D arrays] -> the (B, max(N, 1)) host view holding row b in [b, :len(rows[b])] (clamped to [-1, 1] with `clip`), zero
        beyond.  The view is valid until the next `pack`."""
        if self._copied is not None:
            self._copied.synchronize()
            self._copied = None
        lens = [len(r) for r in rows]
        B, N = len(rows), max(max(lens, default=0), 1)
        if self._buf is None or self._buf.numel() < B * N:
            self._buf = torch.empty(B * N, dtype=torch.float32, pin_memory=torch.cuda.is_available())
        self._view = self._buf[:B * N].view(B, N)
        hv = self._view.numpy()

        def put(b):
            if clip:
                np.clip(rows[b], -1.0, 1.0, out=hv[b, :lens[b]])
            else:
                hv[b, :lens[b]] = rows[b]
            hv[b, lens[b]:] = 0.0
        list(_PACKERS.map(put, range(B)))
        return self._view

    def to(self, device):
        """The packed batch on `device`, by a non-blocking copy on the current stream."""
        y = self._view.to(device, non_blocking=True)
        if y.is_cuda:
            self._copied = torch.cuda.Event()
            self._copied.record(torch.cuda.current_stream(y.device))
        return y


# ------------------------------------------------------------------------------------------------ validation
def require_device(t, who):
    """`t`, a tensor or a torch.device, must be on the GPU.  Returns t."""
    dev = t.device if isinstance(t, torch.Tensor) else t
    if not isinstance(dev, torch.device) or dev.type != "cuda":
        raise RuntimeError(f"{who} runs on an AMD GPU only (no CPU fallback): pass a device tensor or device='cuda'")
    return t


def lengths(lens, B, cap, what, device=None):
    """Per-row lengths (list, numpy array or tensor) of a batch of B rows, each in [0, cap] -> the host list of ints and, when
    `device` is given, (that list, the int32 tensor on the device)."""
    h = [int(v) for v in (lens.tolist() if isinstance(lens, (torch.Tensor, np.ndarray)) else lens)]
    if len(h) != B or any(n < 0 or n > cap for n in h):
        raise ValueError(f"{what} must hold B={B} values in [0, {cap}], got {h}")
    return h if device is None else (h, torch.tensor(h, dtype=torch.int32, device=device))


def rows(x, lens, who, device_lens=True):
    """The input of a ragged launch: x (B, N) float32 on the GPU, row b holding lens[b] samples -> (x contiguous, lens on the host,
    lens int32 on the device, or None without `device_lens`)."""
    require_device(x, who)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"{who}: expected a (B, N) float32 tensor, got {tuple(x.shape)} {x.dtype}")
    x = x.contiguous()
    if not device_lens:
        return x, lengths(lens, x.shape[0], x.shape[1], "lens"), None
    return (x,) + lengths(lens, x.shape[0], x.shape[1], "lens", x.device)
