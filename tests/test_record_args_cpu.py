"""csrc/record_args.hpp — the argument checks the record-buffer entries of the C ABI share — as a plain host program: the header must
compile without HIP (g++ -Wall -Werror, the public header and the standard library only) and give, for every case of
tests/record_args_cases.py, the status the entries gave when each still carried its own copy of the check."""
import os
import subprocess

import record_args_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "cpp", "record_args_harness.cpp")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, HARNESS, "-o", exe])
    ask, want = RC.harness_lines()
    run = subprocess.run([exe], input=ask, capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout, run.stderr)
    got = run.stdout.splitlines()
    assert len(got) == len(want)
    wrong = [(q, g, w) for q, g, w in zip(ask.splitlines(), got, want) if g != w]
    assert not wrong, wrong          # (check, got, expected)
    return run


def test_every_check_gives_the_status_the_entries_gave(tmp_path):
    run = _build_and_run(tmp_path, "record_args_harness", ["-O1"])
    assert f"{len(RC.harness_lines()[1])} checks" in run.stderr


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone binary: 2^31-sized counts, pointer values one past a boundary and offsets at the end of a record go through the
    checks' integer arithmetic without an overflow or a read."""
    run = _build_and_run(tmp_path, "record_args_harness_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr


def test_the_table_covers_what_it_promises():
    """both limits, each at the limit and one above it; every malformed layout named in the module's head"""
    counts = {(lim, n) for (_, n, lim, _), _ in RC.RECORDS}
    assert {("ingest", RC.HALF), ("ingest", RC.HALF + 1), ("map", RC.FULL), ("map", RC.FULL + 1)} <= counts
    assert {(10, 0, 4, 8, -1), (30, 0, 4, 8, 16), (32, 0, 4, 30, 16), (32, 2, 4, 8, 16)} <= set(RC.BAD_XYZ_LAYOUTS)
    assert (32, 0, 4, 8, 30) in RC.BAD_LAYOUTS and (32, 0, 4, 8, 30) not in RC.BAD_XYZ_LAYOUTS
    assert (32, 0, 4, 8, 0) in RC.BAD_OUT_LAYOUTS and (32, 0, 4, 8, 0) not in RC.BAD_LAYOUTS
