"""Side streams of the drivers, cached per process and device: the low-priority stream of iar's convergence checks and the
streams probed for a hardware queue of their own (iar's device eigen-decompositions, contour's node solves).  ONE cache serves
both drivers."""
import ctypes as _C

import torch

from ._lib import lib, check, c_vp, c_i32

_CHECK_STREAMS = {}


def _check_stream():
    dev = torch.cuda.current_device()
    st = _CHECK_STREAMS.get(dev)
    if st is None:
        # the convergence checks are off the critical path: their stream asks for the LOWEST priority the device offers, so that
        # the dispatcher serves the recurrence's kernels first when both streams have work (torch clamps to the device's
        # range, a lower number is a higher priority)
        st = _CHECK_STREAMS[dev] = torch.cuda.Stream(priority=1)
    return st


_EIG_STREAMS = {}


def _eig_streams(count, others=()):
    """streams for the device eigen-decompositions (3 ms one-wavefront kernels) that overlap with the streams in `others`
    (the recurrence's and the checks').  The runtime maps streams onto a small pool of hardware queues and gives no way to ask
    which; two streams on one queue serialise (measured: the convergence checks queued 4 ms per batch behind the
    decompositions).  So candidates are probed (nep_stream_pair_serializes, ~1.5 ms each, once per process and device) and the
    first ones that serialise with none of `others` nor with each other are kept.  Streams already in the cache are handed out
    as they are: they were probed against the `others` of the call that made them, not against this call's."""
    dev = torch.cuda.current_device()
    sts = _EIG_STREAMS.setdefault(dev, [])
    if len(sts) >= count:
        return sts[:count]
    cands = [torch.cuda.Stream(priority=0) for _ in range(8)]
    for c in cands:
        if len(sts) >= count:
            break
        ok = True
        for o in list(others) + sts:
            r = c_i32(0)
            check(lib.nep_stream_pair_serializes(c_vp(o.cuda_stream), c_vp(c.cuda_stream), _C.byref(r)))
            if r.value:
                ok = False
                break
        if ok:
            sts.append(c)
    while len(sts) < count:              # no free hardware queue: better a shared one than none
        sts.append(cands[len(sts) % len(cands)])
        _eig_streams.shared = True
    return sts[:count]


_eig_streams.shared = False
