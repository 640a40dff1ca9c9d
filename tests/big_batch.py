"""Helpers of the tests that run the dense image stages at batch sizes no host array can hold (tests/test_dense_limits_gpu.py,
tests/test_dense_big_gpu.py).  The inputs of such a test are periodic: P distinct items (images, or whole sequences of images)
repeated over the batch on the device, so the numpy restatement runs once for the P items and what the device wrote is compared
with it on the device, byte for byte, over every item of the batch.  An item is everything an array holds for one index of its
first dimension, pad columns included; they must keep the sentinel the array was filled with, or the bytes the input had.  The
last items of a batch may differ from the period (sequences cut short by n_images): they go in and are compared as a `tail`."""
import numpy as np

SENTINEL = 0xA5
SLAB_BYTES = 1 << 28  # of a device array compared at a time; the comparison allocates about 1.25 of it


def need_memory(nbytes):
    """skips the calling test, with the byte counts as the reason, when the device has less free memory than the test needs"""
    import pytest
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip("needs %d bytes of device memory, %d are free" % (nbytes, free))


def release():
    """returns the blocks of the rigs a test has dropped to the device, so that the tests do not stack"""
    import gc

    import torch
    gc.collect()
    torch.cuda.empty_cache()


def sentinel(shape, dtype):
    """a host array of the shape and type whose every byte is the sentinel"""
    return np.full(tuple(shape) + (np.dtype(dtype).itemsize,), SENTINEL, np.uint8).view(dtype).reshape(shape)


def fill_sentinel(*tensors):
    import torch
    for t in tensors:
        if t is not None:
            assert t.is_contiguous()
            t.view(torch.uint8).fill_(SENTINEL)


def periodic(period, n, tail=None, device="cuda"):
    """a contiguous device tensor [n, ...]: item i is period[i % P], but the last len(tail) items, which are tail's.  period and tail
    are host arrays [P, ...] and [T, ...]; nothing of the size of the batch is built on the host"""
    import torch
    period = np.ascontiguousarray(period)
    P = period.shape[0]
    t = torch.from_numpy(period.view(np.uint8).reshape(P, -1)).to(device)
    out = t.repeat(((n + P - 1) // P, 1))[:n]
    if tail is not None and len(tail):
        tail = np.ascontiguousarray(tail)
        out[n - tail.shape[0]:] = torch.from_numpy(tail.view(np.uint8).reshape(tail.shape[0], -1)).to(device)
    dtype = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16, np.dtype(np.int32): torch.int32,
             np.dtype(np.float32): torch.float32}[period.dtype]
    return out.view(dtype).view((n,) + period.shape[1:])


def _first_difference(got, want, first_item, shape, what):
    """got, want: uint8 device tensors [k, item bytes] that differ; -> the message of the assertion"""
    import torch
    k = int(torch.nonzero((got != want).any(dim=1))[0].item())
    g, w = got[k].cpu().numpy(), want[k].cpu().numpy()
    byte = int(np.flatnonzero(g != w)[0])
    item = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
    es = g.size // item
    index = np.unravel_index(byte // es, shape) if len(shape) else ()
    e = byte // es * es
    return "%s: item %d differs first at element %s (byte %d of the item): got %s, want %s" % (
        what, first_item + k, tuple(int(i) for i in index), byte, g[e:e + es].tobytes().hex(), w[e:e + es].tobytes().hex())


def compare_periodic(got, period, what, tail=None):
    """asserts that the device tensor got [n, ...] (contiguous, pad columns included) holds period[i % P] at every item i < n - T
    and tail[j] at item n - T + j, byte for byte; on a mismatch the message names the first item, the element in it, and what was
    got and wanted there.  period, tail: host arrays [P, ...], [T, ...] of got's type and item shape"""
    import torch
    assert got.is_contiguous(), what
    n = int(got.shape[0])
    shape = tuple(got.shape[1:])
    period = np.ascontiguousarray(period)
    assert tuple(period.shape[1:]) == shape and period.dtype.itemsize == got.element_size(), (what, period.shape, tuple(got.shape))
    P = period.shape[0]
    T = 0 if tail is None else len(tail)
    main = n - T
    assert main >= 0
    g = got.view(torch.uint8).reshape(n, -1)
    nb = int(g.shape[1])
    w = torch.from_numpy(period.view(np.uint8).reshape(P, nb)).to(got.device)
    reps = main // P
    step = max(1, SLAB_BYTES // (P * nb))
    for r0 in range(0, reps, step):
        r1 = min(reps, r0 + step)
        slab = g[r0 * P:r1 * P].view(r1 - r0, P, nb)
        if not torch.equal(slab, w.expand(r1 - r0, P, nb)):
            raise AssertionError(_first_difference(slab.reshape(-1, nb), w.repeat((r1 - r0, 1)), r0 * P, shape, what))
    rest = main - reps * P  # the items behind the last whole period
    if rest and not torch.equal(g[reps * P:main], w[:rest]):
        raise AssertionError(_first_difference(g[reps * P:main], w[:rest], reps * P, shape, what))
    if T:
        tail = np.ascontiguousarray(tail)
        assert tuple(tail.shape[1:]) == shape and tail.dtype.itemsize == got.element_size(), (what, tail.shape)
        wt = torch.from_numpy(tail.view(np.uint8).reshape(T, nb)).to(got.device)
        if not torch.equal(g[main:], wt):
            raise AssertionError(_first_difference(g[main:], wt, main, shape, what + " (tail)"))


def compare_sentinel(what, *tensors):
    """asserts that every byte of the device tensors is the sentinel still"""
    import torch
    for i, t in enumerate(tensors):
        if t is None:
            continue
        flat = t.view(torch.uint8).reshape(-1)
        for at in range(0, flat.numel(), SLAB_BYTES):
            part = flat[at:at + SLAB_BYTES]
            if not bool((part == SENTINEL).all()):
                raise AssertionError("%s: array %d was written at byte %d" % (what, i, at + int(torch.nonzero(part != SENTINEL)[0].item())))


def crosses(what, items, item_bytes, P, element_bytes=None, past_elements=False):
    """the two asserts that keep a test of offsets beyond 2^32 bytes honest, for an array of `items` items of item_bytes bytes that
    the stage addresses from its base: (a) the offset of the last item lies at least 4 P items beyond 2^32 bytes (and, with
    past_elements, its element index beyond 2^31); (b) 2^32 bytes are no whole number of items and the item an offset that has
    lost 2^32 lands in is another one of the period: (2^32 // item_bytes) % P != 0, so reading and writing with the same wrapped
    offset cannot cancel out"""
    last = (items - 1) * item_bytes
    assert last >= (1 << 32) + 4 * P * item_bytes, (what, "largest offset", last)
    if past_elements:
        assert last // element_bytes >= (1 << 31) + 4 * P * item_bytes // element_bytes, (what, "largest element", last // element_bytes)
    assert (1 << 32) % item_bytes != 0 and ((1 << 32) // item_bytes) % P != 0, (what, item_bytes, P)
