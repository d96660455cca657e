"""How this project times a call: three methods, two formatters, one record header.  Every tools/time_*.py measures through this module,
except those that tools/notes_measure_once.md lists as left alone.

A step or call time is taken between device events, or with a host clock around work that ends in a device synchronise; every shape is
warmed up before its first timed window; the profiler is off (a kernel trace is a run of its own).  The three methods:

    per_call_events     one pair of device events per call; the window is the call alone
    per_call_host       time.perf_counter around one call plus the device synchronise that ends it
    alternating_rounds  `iters` calls between two device events per round, the implementations taking turns round by round

The clock and the synchronise come from a backend; the default is torch.cuda, a test passes a fake.  The module imports without a GPU and
refuses to measure without one: there is no CPU path."""
import json
import os
import statistics
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class TorchBackend:
    """torch.cuda: event() is a timing event (record(), synchronize(), elapsed_time(later) in ms), synchronize() waits for the device,
    clock() is seconds."""

    def __init__(self):
        import torch
        assert torch.cuda.is_available(), "tools/measure.py measures on the GPU; there is no CPU path"
        self.cuda = torch.cuda

    def event(self):
        return self.cuda.Event(enable_timing=True)

    def synchronize(self):
        self.cuda.synchronize()

    clock = staticmethod(time.perf_counter)


def per_call_events(fn, warmup, repeats, sync_each=False, backend=None):
    """[ms] of `repeats` calls after `warmup` untimed ones.  Inside the window: fn() and nothing else -- its launches, allocations and
    read-backs as a caller pays them -- between two events on the current stream.  A synchronise follows the warm-up and every timed call.
    sync_each=True synchronises before every call too and runs the warm-up calls the way the timed ones run (for a fn that starts from
    what the call before it freed).  fn's result is dropped as soon as it returns."""
    b = backend or TorchBackend()

    def one():
        if sync_each:
            b.synchronize()
        t0, t1 = b.event(), b.event()
        t0.record(); fn(); t1.record()
        b.synchronize()
        return t0.elapsed_time(t1)

    for _ in range(warmup):
        one() if sync_each else fn()
    b.synchronize()
    return [one() for _ in range(repeats)]


def per_call_host(fn, warmup, repeats, backend=None):
    """[ms] of `repeats` calls after `warmup` untimed ones and a synchronise.  Inside the window: fn() and the device synchronise after it,
    on the host clock -- so host work of the call (Python, CPU routes, uploads, read-backs) counts in full."""
    b = backend or TorchBackend()
    for _ in range(warmup):
        fn()
    b.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = b.clock()
        fn()
        b.synchronize()
        ms.append(1e3 * (b.clock() - t0))
    return ms


def alternating_rounds(fns, rounds, iters, warmup, backend=None):
    """{name: [ms per call, one per round]}.  Every fn is called `warmup` times, then one synchronise; then round by round each name that
    has rounds left takes its turn: `iters` calls between two events, a wait for the closing event, window / iters.  The wait is the
    event's own synchronise, not the device's: on the one stream these scripts use both wait for the same work, but the host comes back
    from them differently, and a host-bound window of a few ms that starts after a device synchronise reads higher (measured: see
    tools/notes_measure_once.md).  `rounds` and `iters` are ints or {name: int}; a name with fewer rounds stops taking turns.  One name
    and one round is the plain `N calls between two events`."""
    b = backend or TorchBackend()
    rounds = rounds if isinstance(rounds, dict) else dict.fromkeys(fns, rounds)
    iters = iters if isinstance(iters, dict) else dict.fromkeys(fns, iters)
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    b.synchronize()
    ms = {name: [] for name in fns}
    for r in range(max(rounds.values())):
        for name, fn in fns.items():
            if r >= rounds[name]:
                continue
            t0, t1 = b.event(), b.event()
            t0.record()
            for _ in range(iters[name]):
                fn()
            t1.record()
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1) / iters[name])
    return ms


def stats_ms(samples, key="repeats"):
    """median, min and max in ms rounded to 3 places, and how many samples (`key` is "repeats" or "rounds")"""
    return {"median_ms": round(statistics.median(samples), 3), "min_ms": round(min(samples), 3), "max_ms": round(max(samples), 3), key: len(samples)}


def stats(samples):
    """median, min and max as measured"""
    return {"median": statistics.median(samples), "min": min(samples), "max": max(samples)}


def header():
    """what ties a record to what it measured: the device, the digest of the library's sources, the library's path below the root"""
    import torch
    from streetunveiler_amd import _lib
    from streetunveiler_amd.build import source_digest
    assert torch.cuda.is_available(), "tools/measure.py measures on the GPU; there is no CPU path"
    return {"device": torch.cuda.get_device_name(0), "source_digest": source_digest(), "library": os.path.relpath(_lib.LIB_PATH, ROOT)}


def write_record(path, record):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", path)
