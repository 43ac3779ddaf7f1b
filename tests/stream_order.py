"""Harness of the stream-order tests (tests/test_gpu_stream_order.py, tests/test_gpu_stream_highlevel.py): a call
is handed inputs that its stream is STILL PRODUCING, and the inputs are overwritten on the same stream right
behind it, with no host synchronisation on either side.

    poison everywhere -> [busy(stream)] -> inputs = real -> call() -> inputs = poison -> synchronise

A launch or copy of the call that leaves the stream (the NULL stream, another stream of the library) runs while
the chain is still busy and reads poison; a read the library defers past its last launch on the stream sees
poison too. Poison is always a VALID input of the same shape and type (another seeded field, another array's
integers, another record), so that a misordered run gives wrong bits and nothing else.

A plain module (like tests/mask_model.py): no fixtures, no pytest settings. torch is imported by the functions,
so the module itself imports without a GPU."""

SCRATCH_ELEMS = 32 << 20   # float32: a pass reads and writes 256 MB, tens of microseconds against the few a launch costs the host
CALIBRATE_MS = 20.0
MARGIN = 1.25              # on top of the calibrated chain length

_per_op_ms = None
_scratch = {}


def _scratch_of(stream):
    """One scratch tensor per stream (two chains in flight never write the same memory)."""
    import torch
    key = (stream.device.index, stream.cuda_stream)
    if key not in _scratch:
        if len(_scratch) >= 3:
            raise RuntimeError("stream_order: more than three streams")
        _scratch[key] = torch.zeros(SCRATCH_ELEMS, dtype=torch.float32, device=stream.device)
        torch.cuda.synchronize(stream.device)
    return _scratch[key]


def _chain(x, n):
    for _ in range(n):
        x.add_(0.5)


def _calibrate(stream):
    """Milliseconds of one op of the chain: the chain is doubled until its measured time (torch.cuda.Event)
    reaches CALIBRATE_MS. Once per process."""
    global _per_op_ms
    import torch
    x = _scratch_of(stream)
    n = 32
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            _chain(x, n)
            e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1)
        if t >= CALIBRATE_MS:
            break
        n *= 2
        if n > (1 << 17):
            raise RuntimeError("stream_order: the chain does not reach %g ms" % CALIBRATE_MS)
    _per_op_ms = t / n
    return _per_op_ms


def busy(stream, ms=20):
    """Keeps `stream` busy for at least `ms` milliseconds (a chain of elementwise passes over a scratch tensor,
    its length from the calibration) and returns an event recorded behind the chain."""
    import torch
    if _per_op_ms is None:
        _calibrate(stream)
    n = int(ms * MARGIN / _per_op_ms) + 1
    x = _scratch_of(stream)
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        _chain(x, n)
        ev.record()
    return ev


def warm_up(*streams):
    """Scratch tensors and the calibration, ahead of a test that starts chains on several streams (both
    synchronise the device, which must not happen between two chains)."""
    import torch
    for s in streams:
        busy(s, 0.0)
    torch.cuda.synchronize()


def prepare(inputs, poison, prealloc=()):
    """Step 1 of run_ordered: the work tensors, holding poison, written on the default stream and synchronised.
    prealloc: (output tensor, poison tensor) pairs a case allocated beforehand; they start as poison too."""
    import torch
    assert len(inputs) == len(poison)
    for r, p in zip(inputs, poison):
        assert r.is_cuda and p.is_cuda and r.shape == p.shape and r.dtype == p.dtype, "poison: the input's shape and type"
    work = [torch.empty_like(p) for p in poison]
    for w, p in zip(work, poison):
        w.copy_(p)
    for o, p in prealloc:
        o.copy_(p)
    torch.cuda.synchronize()
    return work


def produce(stream, work, inputs, ms=20):
    """Step 2: `stream` is busy for `ms`, then copies inputs[k] into work[k]. Returns the event behind the copies."""
    import torch
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        busy(stream, ms)
        for w, r in zip(work, inputs):
            w.copy_(r)
        ev.record()
    return ev


def guard(*events):
    """Step 3: the producers must still be running when the call is entered; a test never passes without that."""
    for ev in events:
        if ev.query():
            raise AssertionError("producer finished before the call: delay too short")


def finish(stream, work, poison):
    """Steps 5 and 6: poison again, on the stream, right behind the call; then the one synchronisation."""
    import torch
    try:
        with torch.cuda.stream(stream):
            for w, p in zip(work, poison):
                w.copy_(p)
    finally:
        stream.synchronize()


def run_ordered(stream, inputs, poison, call, ms=20, prealloc=()):
    """inputs / poison: lists of complete device tensors, pairwise of one shape and type (the real values and
    the valid-but-wrong ones). call(*work) gets tensors that hold inputs[k] in stream order only; it runs inside
    `with torch.cuda.stream(stream)` and allocates its outputs there. Returns what call returned, after
    stream.synchronize() (which also happens when the call raises: nothing stays in flight)."""
    import torch
    if _per_op_ms is None:
        warm_up(stream)
    work = prepare(inputs, poison, prealloc)
    ev = produce(stream, work, inputs, ms)
    try:
        with torch.cuda.stream(stream):
            guard(ev)
            out = call(*work)
    finally:
        finish(stream, work, poison)
    return out
