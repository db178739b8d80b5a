"""An index of Gaussian rows normalised to unit length for the perf tools at the dims ssw_index_fill_random does not serve (384, 640, 896,
1152, 1280): torch draws each block of rows on the device and it reaches the index through pinned host memory
(ssw_index_upload takes host rows), so every row is its own draw, as DeviceIndex.synthetic's are."""
import ctypes

DIMS128 = (384, 640, 896, 1152, 1280)


def gaussian_index(n, dim, dtype, seed=2024, block_rows=1 << 17):
    import torch
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    idx = DeviceIndex(n, dim, dtype=dtype)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    host = torch.empty((block_rows, dim), dtype=torch.float32).pin_memory()
    for r0 in range(0, n, block_rows):
        m = min(block_rows, n - r0)
        x = torch.randn((m, dim), generator=gen, device="cuda")
        x /= x.norm(dim=1, keepdim=True)
        host[:m].copy_(x)
        _lib.call("ssw_index_upload", idx._h, ctypes.c_void_p(host.data_ptr()), r0, m)
    del host
    torch.cuda.empty_cache()
    return idx


def make_index(n, dim, dtype, seed=2024):
    """DeviceIndex.synthetic where the device can fill the rows, gaussian_index at the dims of DIMS128"""
    from seesaw_amd.device_index import DeviceIndex
    return gaussian_index(n, dim, dtype, seed) if dim in DIMS128 else DeviceIndex.synthetic(n, dim, seed=seed, dtype=dtype)
