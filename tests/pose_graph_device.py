"""What the pose graph's GPU tests share (test_pose_graph_gpu.py, test_pose_graph_robust_gpu.py, test_pose_graph_place_gpu.py,
test_pose_graph_loops_gpu.py): buffers between guards, byte equality, and the measurement that a chain of calls does not wait for the
device."""
import math
import time

import numpy as np
import pytest

GUARD = 256                                    # bytes in front of and behind every buffer
FILL = 0x5A
INV = 1                                        # LSD_ERR_INVALID


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """The bytes of `a` on the device with GUARD bytes of the fill pattern on either side."""

    def __init__(self, a):
        self.raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()
        pad = np.full(GUARD, FILL, np.uint8)
        self.t = dev(np.concatenate([pad, self.raw, pad]))
        self.ptr = self.t.data_ptr() + GUARD

    def back(self):
        """(the bytes now, True if both guards are untouched)."""
        a = self.t.cpu().numpy()
        n = len(self.raw)
        return a[GUARD:GUARD + n], bool((a[:GUARD] == FILL).all() and (a[GUARD + n:] == FILL).all())

    def unchanged(self):
        got, ok = self.back()
        return ok and got.tobytes() == self.raw.tobytes()


def filled(n_bytes):
    return Guarded(np.full(n_bytes, FILL, np.uint8))


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def same(got, want):
    return np.ascontiguousarray(got).view(np.uint8).tobytes() == np.ascontiguousarray(want).view(np.uint8).tobytes()


def returns_in_front_of_the_device(run, calls):
    """run() -- a chain the caller has run once already, so that every workspace has its size -- with ~80 ms of work in front of it on the
    stream, warmed and sized on this device: it must return while that work is still running.  calls: the names of what run() calls,
    for the message.  Skips where the stream drained before run() was called; synchronised on return, so that the caller can check
    what run() left."""
    import torch
    a = torch.randn(4096, 4096, device="cuda")

    def burn(count):
        for _ in range(count):
            a @ a
    burn(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    burn(10)
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / 10
    count = max(10, min(5000, int(math.ceil(0.08 / per))))                             # ~80 ms of work in front of the chain
    done = torch.cuda.Event()
    burn(count)
    done.record()
    if done.query():
        pytest.skip("the stream drained before the calls were made (%d matmuls of %.3f ms): the host was too slow to tell" % (count, per * 1e3))
    run()
    still_running = not done.query()
    torch.cuda.synchronize()
    assert still_running, calls + " returned only after the work in front of them had finished"
