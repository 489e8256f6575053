"""The delayed producer: does a call run ENTIRELY on the stream it was made on?

``delayed(call, real, poison)``:
1. allocates the call's input tensors and, on the default stream, fills them with ``poison`` - benign values: in-range
   indices, finite or NaN floats, valid row ids that give different results, never an out-of-range value - and
   synchronises;
2. on a side stream ``s`` enqueues a delay kernel (``torch.cuda._sleep``, about DELAY_MS);
3. still on ``s``, copies the ``real`` inputs (device-resident copies) over the poison and makes the call;
4. right after the call returns, notes whether ``s`` is still busy (``not s.query()``): if it is, the delay was running
   while every launch of the call was enqueued, so nothing of the call had started when the last launch was made;
5. clones the outputs on ``s``, synchronises ``s`` and returns them with that flag.

A kernel, memset or copy that the call issues on any other stream runs before its inputs exist - it reads the poison, or
its output is overwritten by work that should have come first - and the result differs from the same call made on the
default stream.  ``stray`` (the control): a function run on the DEFAULT stream inside the window; it must see the poison.

A call that synchronises with the host cannot be delayed this way (step 4 fails, and fails the case: it does not skip);
``on_stream(call)`` runs such a call under ``s`` without the delay, for stream-independence of results only.
"""
import torch

DELAY_MS = 50.0            # the documented host enqueue time of a request is 0.4 to 1.8 ms; the busy flag is the guard
_state = {}


def side_stream(device="cuda"):
    """The one side stream of the session (with the default stream: 2 of the 4 hardware queues a process opens)."""
    if "stream" not in _state:
        _state["stream"] = torch.cuda.Stream(device)
    return _state["stream"]


def delay_cycles():
    """``torch.cuda._sleep`` cycles for about DELAY_MS, calibrated once per session with events."""
    if "cycles" not in _state:
        probe = 2_000_000
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(probe)                                      # (first launch: module load)
        a.record()
        torch.cuda._sleep(probe)
        b.record()
        b.synchronize()
        _state["cycles"] = max(probe, int(probe * DELAY_MS / max(a.elapsed_time(b), 1e-3)))
    return _state["cycles"]


def tree_map(fn, x):
    if isinstance(x, torch.Tensor):
        return fn(x)
    if isinstance(x, dict):
        return {k: tree_map(fn, v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(tree_map(fn, v) for v in x)
    return x


def first_difference(got, ref, path="out"):
    """None when the two trees hold the same bits (NaNs compare by bit pattern), else where they differ first."""
    if isinstance(ref, torch.Tensor):
        if not isinstance(got, torch.Tensor) or got.shape != ref.shape or got.dtype != ref.dtype:
            return f"{path}: {getattr(got, 'shape', got)} {getattr(got, 'dtype', '')} != {ref.shape} {ref.dtype}"
        g, r = (t.detach().contiguous().reshape(-1).view(torch.uint8).cpu() for t in (got, ref))
        if not torch.equal(g, r):
            bad = (g != r).nonzero()
            return f"{path}: {bad.numel()} of {g.numel()} bytes differ, first at byte {int(bad[0])}"
        return None
    if isinstance(ref, dict):
        if not isinstance(got, dict) or set(got) != set(ref):
            return f"{path}: keys differ"
        for k in ref:
            d = first_difference(got[k], ref[k], f"{path}[{k!r}]")
            if d:
                return d
        return None
    if isinstance(ref, (list, tuple)):
        if not isinstance(got, (list, tuple)) or len(got) != len(ref):
            return f"{path}: lengths differ"
        for i, (g, r) in enumerate(zip(got, ref)):
            d = first_difference(g, r, f"{path}[{i}]")
            if d:
                return d
        return None
    return None if got == ref else f"{path}: {got!r} != {ref!r}"


def delayed(call, real, poison, stray=None):
    """``call(**inputs)`` behind the delay (module docstring).  ``real`` / ``poison``: {name: device tensor}, same shapes
    and dtypes.  -> (the outputs, cloned; was ``s`` still busy when the call returned; what ``stray(inputs)`` returned)."""
    assert set(real) == set(poison)
    s, cycles = side_stream(), delay_cycles()
    bufs = {k: torch.empty_like(v) for k, v in real.items()}
    for k, v in bufs.items():
        assert poison[k].shape == v.shape and poison[k].dtype == v.dtype, k
        v.copy_(poison[k])
    torch.cuda.synchronize()
    seen = None
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        for k, v in bufs.items():
            v.copy_(real[k])
        out = call(**bufs)
        busy = not s.query()
        if stray is not None:
            with torch.cuda.stream(torch.cuda.default_stream()):
                seen = tree_map(torch.clone, stray(bufs))
        out = tree_map(torch.clone, out)
    s.synchronize()
    torch.cuda.synchronize()
    return out, busy, seen


def on_stream(call):
    """``call()`` under the side stream, no delay -> its outputs, cloned, after the stream has drained."""
    s = side_stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = tree_map(torch.clone, call())
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    return out


def check_delayed(call, ref_call, real, poison):
    """The standard case: ``ref_call(**real)`` on the default stream against ``call`` behind the delay -> asserts that the
    stream was still busy and that the outputs are the same bits.  (``call`` and ``ref_call`` act on fresh twins.)"""
    ref = tree_map(torch.clone, ref_call(**real))
    torch.cuda.synchronize()
    out, busy, _ = delayed(call, real, poison)
    assert busy, "the side stream was idle when the call returned: the call waited for the device (or the delay is too short)"
    why = first_difference(out, ref)
    assert why is None, "on the side stream, behind a delayed producer: " + why
    return out
