"""Guard bands for the GPU tests that call the C ABI with every buffer at its EXACT size (the idea of tests/test_gpu_guard.py, for hand-carved buffers
instead of torch's allocation functions): a buffer is a slice of a larger allocation whose bytes right before and right after it hold a pattern; a
kernel that rounds a store up, writes a tail element or mis-sizes a workspace damages them.  Self-test: tests/test_gpu_guard.py."""
import numpy as np
import torch

PRE, POST, PATTERN = 512, 4096, 0xA5             # PRE keeps the buffer at the alignment torch's allocator gives (512 B); the kernels assume 16 B


class Guard:
    def __init__(self, dev):
        self.dev, self.live = dev, []             # live: (raw uint8 tensor, payload bytes, what)

    def buf(self, nbytes=None, what="", src=None):
        """a guarded buffer of ``nbytes`` bytes of the pattern, or one holding the bytes of the numpy array ``src`` (which may come first); the first
        canary byte comes right after it"""
        if src is None and isinstance(nbytes, np.ndarray):
            src, nbytes = nbytes, None
        nbytes = src.nbytes if src is not None else nbytes
        raw = torch.full((PRE + nbytes + POST,), PATTERN, dtype=torch.uint8, device=self.dev)
        if src is not None and nbytes:
            raw[PRE:PRE + nbytes] = torch.from_numpy(np.ascontiguousarray(src).reshape(-1).view(np.uint8).copy()).to(self.dev)
        self.live.append((raw, nbytes, what))
        return raw[PRE:PRE + nbytes]

    def damaged(self):
        torch.cuda.synchronize()
        return [(what, n) for raw, n, what in self.live if not (bool((raw[:PRE] == PATTERN).all()) and bool((raw[PRE + n:] == PATTERN).all()))]
