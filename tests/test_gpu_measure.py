"""GPU (-m gpu): tools/measure.py with its real backend on a 1 Mi-element torch.add.  Each method returns the number of samples it was asked
for, finite and positive; the same function under two names alternates to medians of the same order of magnitude.  A sanity check of the
plumbing: no time is held to a tolerance."""
import math
import statistics

import pytest
import torch

from tools import measure

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def add():
    a, b = torch.rand(1 << 20, device="cuda:0"), torch.rand(1 << 20, device="cuda:0")
    return lambda: torch.add(a, b)


def _sane(samples, count):
    assert len(samples) == count and all(math.isfinite(t) and t > 0 for t in samples), samples


@pytest.mark.parametrize("sync_each", [False, True])
def test_per_call_events(add, sync_each):
    _sane(measure.per_call_events(add, warmup=2, repeats=9, sync_each=sync_each), 9)


def test_per_call_host(add):
    _sane(measure.per_call_host(add, warmup=2, repeats=9), 9)


def test_alternating_rounds(add):
    ms = measure.alternating_rounds({"one": add, "other": add}, rounds={"one": 7, "other": 5}, iters=50, warmup=3)
    _sane(ms["one"], 7)
    _sane(ms["other"], 5)
    ratio = statistics.median(ms["one"]) / statistics.median(ms["other"])
    print("medians, ms per call:", statistics.median(ms["one"]), statistics.median(ms["other"]))
    assert 0.1 < ratio < 10.0                    # the same function: the same order of magnitude


def test_header_names_the_device_and_the_library():
    h = measure.header()
    assert sorted(h) == ["device", "library", "source_digest"] and h["device"] == torch.cuda.get_device_name(0)
