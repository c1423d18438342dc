"""The measurement frame under the per-op A/B tools (tools/_bench.py), without a GPU: the ship rule on made-up lists, the
switch flip, the JSON writer, and the child driver against a stub child written here.

The rule sets shipped defaults and the driver decides whether a tool starts another process after one has failed, so
every assertion is exact: floats that are sums of binary fractions, strings, file contents.  The stub child imports no
torch; no test starts more than one child at a time."""
import json
import os
import sys
import textwrap
import time
import types

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import _bench  # noqa: E402


# ---------------------------------------------------------------------------------------------------------- the rule

def test_leg_summary():
    assert _bench.leg_summary([2.0, 4.0, 3.0]) == {"mean": 3.0, "spread": 2.0, "min": 2.0, "max": 4.0}
    assert _bench.leg_summary([5.0]) == {"mean": 5.0, "spread": 0.0, "min": 5.0, "max": 5.0}


@pytest.mark.parametrize("case, kernel, other, wins", [
    ("a clear win", [1.0, 1.5, 1.25], [9.0, 10.0, 11.0], True),
    ("a win smaller than the other leg's spread", [9.0, 9.0, 9.0], [9.0, 10.0, 11.0], False),          # 1 > 2
    ("a difference exactly equal to the spread", [8.0, 8.0, 8.0], [9.0, 10.0, 11.0], False),           # strict: 2 > 2
    ("the same with two repeats", [8.0, 8.0], [9.0, 11.0], False),
    ("just past the spread", [7.75, 8.0], [9.0, 11.0], True),                                          # 2.125 > 2
    ("a single repeat: the spread is 0", [3.0], [3.5], True),
    ("a single repeat, equal", [3.0], [3.0], False),
    ("the kernel leg slower", [12.0, 12.0, 12.0], [9.0, 10.0, 11.0], False),
    ("the kernel leg slower, single repeat", [4.0], [3.5], False),
])
def test_beats(case, kernel, other, wins):
    assert _bench.beats(kernel, other) is wins, case
    # the rule as the tools spelled it out: mean(ref) - mean(hip) > max(ref) - min(ref)
    assert wins == (sum(other) / len(other) - sum(kernel) / len(kernel) > max(other) - min(other))


# -------------------------------------------------------------------------------------------------------- the switch

def test_switched_restores():
    mod = types.SimpleNamespace(ENABLED="default", OTHER=1)
    with _bench.switched(mod, "ENABLED", False):
        assert mod.ENABLED is False
    assert mod.ENABLED == "default" and mod.OTHER == 1


def test_switched_restores_after_an_exception():
    mod = types.SimpleNamespace(ENABLED=True)
    with pytest.raises(KeyError):
        with _bench.switched(mod, "ENABLED", False):
            assert mod.ENABLED is False
            raise KeyError("inside the block")
    assert mod.ENABLED is True


def test_switched_nests_in_order():
    mod = types.SimpleNamespace(ENABLED=0)
    with _bench.switched(mod, "ENABLED", 1):
        with _bench.switched(mod, "ENABLED", 2):
            with pytest.raises(ValueError):
                with _bench.switched(mod, "ENABLED", 3):
                    assert mod.ENABLED == 3
                    raise ValueError
            assert mod.ENABLED == 2
        assert mod.ENABLED == 1
    assert mod.ENABLED == 0


def test_alternate_order_of_calls():
    mod = types.SimpleNamespace(ENABLED=None)
    calls = []

    def measure(tag):
        def fn(on):
            calls.append((tag, on, mod.ENABLED))
            return float(len(calls))
        return fn

    runs = _bench.alternate(2, {"hip": True, "torch": False}, {"forward": measure("f"), "step": measure("s")},
                            entering=lambda on: _bench.switched(mod, "ENABLED", on))
    assert calls == [(tag, on, on) for _ in range(2) for on in (True, False) for tag in ("f", "s")]
    assert runs == {"hip": {"forward": [1.0, 5.0], "step": [2.0, 6.0]}, "torch": {"forward": [3.0, 7.0], "step": [4.0, 8.0]}}
    assert list(runs) == ["hip", "torch"] and list(runs["hip"]) == ["forward", "step"]
    assert mod.ENABLED is None
    assert _bench.alternate(1, {"a": 2.0}, {"m": lambda arg: arg}) == {"a": {"m": [2.0]}}


# -------------------------------------------------------------------------------------------------------- the writer

def test_write_json(tmp_path):
    path = tmp_path / "not" / "there" / "yet" / "out.json"
    result = {"workload": "text", "shapes": [{"n": 1, "ms": [0.5, 0.25]}], "ships_enabled": False, "none": None}
    _bench.write_json(str(path), result)
    text = path.read_text()
    assert text == json.dumps(result, indent=1) + "\n"
    assert text.endswith("}\n") and not text.endswith("\n\n") and '\n "workload"' in text
    assert json.loads(text) == result
    _bench.write_json(str(path), {"second": 1})                     # rewritten, not appended to
    assert json.loads(path.read_text()) == {"second": 1}


# -------------------------------------------------------------------------------------------------------- the driver

STUB = textwrap.dedent('''\
    import argparse
    import json
    import sys
    import time
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--log")
    ap.add_argument("--behave", default="{}")
    ap.add_argument("--factor", type=int, default=1)
    a = ap.parse_args()
    with open(a.log, "a") as fh:
        fh.write(a.child + "\\n")
    how = json.loads(a.behave).get(a.child, "ok")
    if how == "exit 3":
        sys.exit(3)
    if how == "sleep":
        time.sleep(30)
    print("a line that is no result")
    if how != "silent":
        print("RESULT " + json.dumps({"unit": a.child, "value": a.factor * len(a.child)}), flush=True)
    print("another line after it")
''')


def run_driver(tmp_path, behave, limit=20.0):
    """``drive`` over the units a, bb, ccc -> (the SystemExit or None, units started, ``--out`` as read in every
    ``collect``, the final ``--out`` or None, seconds)."""
    stub, log, out = tmp_path / "stub_child.py", tmp_path / "started.log", tmp_path / "deep" / "out.json"
    stub.write_text(STUB)
    result = {"workload": "stub", "units": []}
    seen = []

    def collect(unit, payload):
        seen.append(json.loads(out.read_text()) if out.exists() else None)
        assert payload["unit"] == unit
        result["units"].append(payload)

    t0, failure = time.monotonic(), None
    try:
        _bench.drive(str(stub), ["a", "bb", "ccc"], ["--log", log, "--behave", json.dumps(behave), "--factor", 10], limit,
                     str(out), result, collect)
    except SystemExit as exc:
        failure = exc
    started = log.read_text().split()
    return failure, started, seen, json.loads(out.read_text()) if out.exists() else None, time.monotonic() - t0


def test_drive_all_units(tmp_path):
    failure, started, seen, final, _ = run_driver(tmp_path, {})
    entries = [{"unit": "a", "value": 10}, {"unit": "bb", "value": 20}, {"unit": "ccc", "value": 30}]
    assert failure is None and started == ["a", "bb", "ccc"]
    assert final == {"workload": "stub", "units": entries}
    # --out as it stood when each unit came back: rewritten after every unit before it
    assert seen == [None, {"workload": "stub", "units": entries[:1]}, {"workload": "stub", "units": entries[:2]}]


def stopped_at_the_second(failure, started, seen, final):
    assert isinstance(failure, SystemExit) and failure.code not in (None, 0)
    assert "stub_child.py" in str(failure.code) and ": bb:" in str(failure.code) and "nothing more is started" in str(failure.code)
    assert started == ["a", "bb"]                                   # the third was never started
    assert final == {"workload": "stub", "units": [{"unit": "a", "value": 10}]}
    assert seen == [None]


def test_drive_stops_after_a_failing_child(tmp_path):
    failure, started, seen, final, _ = run_driver(tmp_path, {"bb": "exit 3"})
    stopped_at_the_second(failure, started, seen, final)
    assert "status 3" in str(failure.code)


def test_drive_stops_after_a_child_without_a_result_line(tmp_path):
    failure, started, seen, final, _ = run_driver(tmp_path, {"bb": "silent"})
    stopped_at_the_second(failure, started, seen, final)
    assert "0 result lines" in str(failure.code)


def test_drive_stops_after_a_child_out_of_time(tmp_path):
    failure, started, seen, final, seconds = run_driver(tmp_path, {"bb": "sleep"}, limit=1.0)
    stopped_at_the_second(failure, started, seen, final)
    assert "timed out" in str(failure.code)
    assert seconds < 10.0, seconds                                  # a cap against a hanging test: the child was killed


def test_run_child_passes_the_environment(tmp_path):
    script = tmp_path / "env_child.py"
    script.write_text("import os\nimport sys\nsys.exit(5) if 'BENCH_FRAME_SWITCH' not in os.environ else "
                      "print(os.environ['BENCH_FRAME_SWITCH'])\n")
    out = _bench.run_child("tool.py", "unit", [sys.executable, str(script)], 20.0, env=dict(os.environ, BENCH_FRAME_SWITCH="0"))
    assert out == "0\n"
    with pytest.raises(SystemExit, match="tool.py: unit: .*nothing more is started"):
        _bench.run_child("tool.py", "unit", [sys.executable, str(script)], 20.0,
                         env={k: v for k, v in os.environ.items() if k != "BENCH_FRAME_SWITCH"})
