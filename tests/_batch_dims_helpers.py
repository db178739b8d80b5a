"""Test infrastructure of tests/test_topk_batch_dims_gpu.py: the hard rows and queries of tests/test_topk_batch_gpu.py
(copied, so that no test module is imported by another), a ragged image map, and one rank of the batched sharded
exchange.  Never imported by the product."""
import ctypes

import numpy as np

F16 = np.float16


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def widen(X):
    return np.asarray(X).astype(np.float16).astype(np.float32)


def hard_rows(oracle, n, dim, seed):
    """unit rows scaled to general magnitudes, with elements in the f16 subnormal range and exact
    round-to-nearest-even ties"""
    rng = np.random.default_rng(seed)
    X = oracle.synth_rows(seed, 0, n, dim) * rng.uniform(0.25, 40.0, size=(n, 1)).astype(np.float32)
    m = rng.random(X.shape)
    X[m < 0.05] = (rng.standard_normal(int((m < 0.05).sum())) * 3e-6).astype(np.float32)  # subnormal in f16
    ties = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(2 + 2.0 ** -10), 2.0 ** -25, 3 * 2.0 ** -25,
                     -5 * 2.0 ** -25, 2.0 ** -14 + 2.0 ** -25, 0.5 + 2.0 ** -12], dtype=np.float32)
    sel = (m >= 0.05) & (m < 0.08)
    X[sel] = ties[rng.integers(0, ties.shape[0], int(sel.sum()))]
    return np.ascontiguousarray(X, dtype=np.float32)


def queries(oracle, nq, dim, first=0):
    return np.stack([oracle.synth_query(first + i, dim) * np.float32(1.0 + 0.1 * i) for i in range(nq)])


def ragged(n_images, lo, hi, seed):
    counts = np.random.default_rng(seed).integers(lo, hi, size=n_images)
    return np.repeat(np.arange(n_images), counts).astype(np.int32)


def expected_launches(nq, width):
    """chunks of `width`, then the narrower powers of two, at last a single query: one scan launch each"""
    return nq // width + bin(nq % width).count("1")


def launches_of(idx, fn):
    """(fn(), the event pairs it recorded on the handle: one per scan launch)"""
    idx.profile(True)
    try:
        out = fn()
        return out, int(idx.profile_read().shape[0])
    finally:
        idx.profile(False)


class OneRank:
    """a handle as the only rank of the batched sharded exchange: its message block, and the merge launch over it"""

    def __init__(self, handle, n_slots, k_max):
        import torch
        self.torch, self.h, self.n_slots, self.k_max = torch, handle, n_slots, k_max
        self.dev = torch.device("cuda", 0)
        self.msg_len = 2 * k_max + 1  # with best rows
        handle.set_stream(torch.cuda.current_stream(self.dev).cuda_stream)
        self.block = torch.full((n_slots, self.msg_len), -1, dtype=torch.int64, device=self.dev)
        handle.set_exchange_target_batch(self.block.data_ptr(), n_slots, k_max, True, 0, 0)

    def merge(self, nq, k):
        """(keys u64 [nq, k_max], counts, flags) of one merge launch over the world of one"""
        torch = self.torch
        from seesaw_amd import _lib
        gathered = self.block[:nq].reshape(1, nq, self.msg_len).contiguous()
        keys = torch.zeros((nq, self.k_max), dtype=torch.int64, device=self.dev)
        counts = torch.zeros(nq, dtype=torch.int32, device=self.dev)
        flags = torch.full((nq, 1), -1, dtype=torch.int64, device=self.dev)
        seen = torch.zeros(1, dtype=torch.int64, device=self.dev)
        _lib.call("ssw_topk_merge_msgs_batch_dev", 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                  ctypes.c_void_p(gathered.data_ptr()), 1, nq * self.msg_len, nq, self.k_max, 1, k,
                  ctypes.c_void_p(keys.data_ptr()), ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(flags.data_ptr()),
                  ctypes.c_void_p(seen.data_ptr()))
        torch.cuda.synchronize()
        return keys.cpu().numpy().view(np.uint64), counts.cpu().numpy(), flags.cpu().numpy()
