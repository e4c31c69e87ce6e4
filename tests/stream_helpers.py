"""Helpers of tests/test_gpu_streams.py: a calibrated GPU delay and inputs that arrive late on a side stream.

A kernel that is enqueued on the wrong stream (or an op that reads memory another stream still owns) shows only when the
right stream is BUSY: delay() keeps a stream busy for a known time, late() puts the real input bytes behind that delay.
Until they arrive the tensors hold zero bytes, which every operator accepts (index 0 is in range, all-zero row splits are
empty rows, points at the origin are duplicates): a kernel that runs too early computes a wrong result and follows no
bad index."""
import torch

_cycles_per_ms = None


def _calibrate():
    """spin cycles of torch.cuda._sleep per millisecond, measured once per session with two timed events"""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        probe = 20_000_000
        ms = 0.0
        for _ in range(2):  # the first launch pays for loading the kernel
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            torch.cuda._sleep(probe)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
        assert ms > 0.5, "torch.cuda._sleep(%d) took %.3f ms: no usable delay on this device" % (probe, ms)
        _cycles_per_ms = probe / ms
    return _cycles_per_ms


def delay(stream, ms=30.0):
    """keeps `stream` busy for about `ms` milliseconds -> an event recorded behind the delay.  The length is no tolerance:
    the tests assert on the event (still pending when an asynchronous op has returned) that it was long enough."""
    cycles = int(ms * _calibrate())
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def late(stream, *good, ms=30.0):
    """-> ([tensors], event): for every tensor of `good` (None passes through) a tensor of its shape and dtype whose bytes
    are all zero now and become `good`'s on `stream`, behind one delay(); the event is that delay's."""
    out = [None if g is None else torch.zeros_like(g, memory_format=torch.contiguous_format) for g in good]
    torch.cuda.synchronize()
    ev = delay(stream, ms)
    with torch.cuda.stream(stream):
        for o, g in zip(out, good):
            if o is not None:
                o.copy_(g, non_blocking=True)
    return out, ev


def late_inplace(stream, *tensors, ms=30.0):
    """late() on the tensors' own storage (for inputs something else already points to, such as the arrays of a ConvPlan):
    zeroed now, their bytes come back on `stream` behind one delay() -> that delay's event"""
    keep = [t.clone() for t in tensors]
    for t in tensors:
        t.zero_()
    torch.cuda.synchronize()
    ev = delay(stream, ms)
    with torch.cuda.stream(stream):
        for t, k in zip(tensors, keep):
            t.copy_(k, non_blocking=True)
    return ev, keep  # (`keep` must outlive the copies: the caller holds it until it has synchronised)
