"""tools/measure.py on the CPU, with a fake backend whose clock is a script: which calls are sampled, where the synchronises fall, how the
implementations take turns, what the formatters and the record writer give, and that every timing script of tools/ goes through the
module -- the list of those that do not is read from tools/notes_measure_once.md, so it cannot rot."""
import glob
import json
import os
import re
import statistics
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import measure  # noqa: E402

ARGPARSE_REWRITTEN = ("time_mesh", "time_tsdf", "time_densify", "time_mesh_post", "time_cluster", "time_knn")


class FakeBackend:
    """Device time only moves when a timed function runs: call number i (from 1) takes i ms.  The log holds everything in order."""

    def __init__(self):
        self.now, self.calls, self.log = 0.0, 0, []

    def fn(self, name="call"):
        def run():
            self.calls += 1
            self.now += self.calls
            self.log.append(name)
        return run

    def event(self):
        backend = self

        class Event:
            def record(self):
                self.at = backend.now
                backend.log.append("record")

            def synchronize(self):
                backend.log.append("sync")

            def elapsed_time(self, later):
                return later.at - self.at
        return Event()

    def synchronize(self):
        self.log.append("sync")

    def clock(self):
        return self.now / 1e3


@pytest.mark.parametrize("sync_each", [False, True])
def test_per_call_events_samples_only_the_repeats(sync_each):
    b = FakeBackend()
    ms = measure.per_call_events(b.fn(), warmup=2, repeats=3, sync_each=sync_each, backend=b)
    assert b.calls == 5 and ms == [3.0, 4.0, 5.0]                      # calls 1 and 2 are the warm-up
    timed = ["sync"] * sync_each + ["record", "call", "record", "sync"]
    assert b.log[-3 * len(timed):] == timed * 3
    if sync_each:
        assert b.log == timed * 2 + ["sync"] + timed * 3               # the warm-up calls run the way the timed ones do
    else:
        assert b.log == ["call", "call", "sync"] + timed * 3


def test_per_call_host_samples_only_the_repeats():
    b = FakeBackend()
    ms = measure.per_call_host(b.fn(), warmup=2, repeats=3, backend=b)
    assert b.calls == 5 and ms == pytest.approx([3.0, 4.0, 5.0])
    assert b.log == ["call", "call", "sync"] + ["call", "sync"] * 3


def test_alternating_rounds_take_turns():
    b = FakeBackend()
    ms = measure.alternating_rounds({"A": b.fn("A"), "B": b.fn("B")}, rounds=2, iters=3, warmup=1, backend=b)
    window = lambda name: ["record"] + [name] * 3 + ["record", "sync"]
    assert b.log == ["A", "B", "sync"] + window("A") + window("B") + window("A") + window("B")
    # calls 1, 2 warm; A's first window is calls 3, 4, 5, B's 6, 7, 8, and so on: each sample is its window over iters
    assert ms == {"A": [(3 + 4 + 5) / 3, (9 + 10 + 11) / 3], "B": [(6 + 7 + 8) / 3, (12 + 13 + 14) / 3]}


def test_alternating_rounds_per_name_rounds_and_iters():
    b = FakeBackend()
    ms = measure.alternating_rounds({"A": b.fn("A"), "B": b.fn("B")}, rounds={"A": 3, "B": 1}, iters={"A": 2, "B": 1}, warmup=0, backend=b)
    turns = [x for x in b.log if x in "AB"]
    assert turns == ["A", "A", "B", "A", "A", "A", "A"]                # B stops taking turns after its one round
    assert ms == {"A": [(1 + 2) / 2, (4 + 5) / 2, (6 + 7) / 2], "B": [3.0]}


def test_formatters_reproduce_the_old_formulas():
    v = [1.23456, 9.87654, 2.00049, 2.0005]
    assert measure.stats_ms(v) == {"median_ms": round(statistics.median(v), 3), "min_ms": 1.235, "max_ms": 9.877, "repeats": 4}
    assert list(measure.stats_ms(v, key="rounds")) == ["median_ms", "min_ms", "max_ms", "rounds"]
    assert measure.stats(v) == {"median": statistics.median(v), "min": 1.23456, "max": 9.87654}


def test_header_and_write_record(tmp_path, monkeypatch, capsys):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "get_device_name", lambda i: "a device")
    h = measure.header()
    assert sorted(h) == ["device", "library", "source_digest"] and not os.path.isabs(h["library"])
    record = {"device": h["device"], "rows": [{"median_ms": 1.5}], "note": None}
    path = tmp_path / "not" / "there" / "yet.json"
    measure.write_record(str(path), record)
    assert json.load(open(path)) == record and "wrote" in capsys.readouterr().out


def test_no_cpu_path(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for method in (lambda: measure.per_call_events(lambda: None, 0, 1), lambda: measure.per_call_host(lambda: None, 0, 1),
                   lambda: measure.alternating_rounds({"a": lambda: None}, 1, 1, 0), measure.header):
        with pytest.raises(AssertionError, match="measures on the GPU; there is no CPU path"):
            method()


def _notes_lists():
    """(scripts the notes name under a method, scripts the notes say were left alone)"""
    notes = open(os.path.join(ROOT, "tools", "notes_measure_once.md")).read()
    methods = notes.split("## Which script uses which method")[1].split("\n## ")[0]
    alone = notes.split("## Left alone")[1].split("\n## ")[0]
    names = lambda text: set(re.findall(r"`(\w+)\.py`", text))
    return names(methods), names(alone)


def test_every_timing_loop_of_tools_is_the_module_or_a_named_exception():
    converted, alone = _notes_lists()
    timing = re.compile(r"perf_counter|Event\(enable_timing")
    source = {os.path.basename(p)[:-3]: open(p).read() for p in glob.glob(os.path.join(ROOT, "tools", "*.py"))}
    assert {name for name, text in source.items() if timing.search(text)} == alone | {"measure"}
    assert len(converted) >= 27 and not converted & alone and set(ARGPARSE_REWRITTEN) <= converted
    for name in converted:
        assert "from tools import measure" in source[name], name
    assert {name for name, text in source.items() if "from tools import measure" in text} == converted


def test_rewritten_argument_parsing_without_a_gpu():
    """--help exits 0 and an unknown flag exits non-zero, before anything touches a device (none is visible to these processes)"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    run = lambda name, flag: subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", name + ".py"), flag], env=env, cwd=ROOT,
                                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    started = [(name, flag, run(name, flag)) for name in ARGPARSE_REWRITTEN for flag in ("--help", "--no-such-flag")]
    for name, flag, p in started:
        out, err = p.communicate()
        if flag == "--help":
            assert p.returncode == 0 and "usage:" in out, (name, err[-500:])
        else:
            assert p.returncode == 2 and "unrecognized arguments" in err, (name, p.returncode, err[-500:])
