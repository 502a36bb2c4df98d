"""The verify pipeline's tick planner (csrc/bp_tick_plan.h: the stage table, plan_tick, lane_sort_sets)
run on the CPU by tests/tick_plan_check.hip, a stand-alone host program:

* replay: every scenario of tests/golden/tick_plans.json (the plans the library launched before the
  planner was split out of Pipeline::push; tests/golden/tick_plans.README.md) gives the recorded
  rows exactly: tick form, region count, total and every region's (kind, slot, r, begin, items);
  the lane sort's sets and blocks; the pipeline depth.
* sweep: the planner's invariants over n = 1 .. 65536, every mode, L_len, tree form, split stage 0
  where it applies, B in {1, 63, 64, 1000}, full and draining pipelines; once more under
  AddressSanitizer + UndefinedBehaviourSanitizer (host code only, nothing loaded into Python)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tick_plan_check.hip")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")


def _build(exe, opt, extra=()):
    subprocess.run(["hipcc", opt, "-std=c++17", "--cuda-host-only", "-x", "hip", SRC, "-o", str(exe)] + list(extra),
                   check=True, capture_output=True)
    return str(exe)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("tick_plan") / "tpc", "-O2")


def _rows(text):
    out = []
    for ln in text.splitlines():
        w = ln.split()
        v = [int(x) for x in w[1:]]
        if w[0] == "tick":
            out.append(["tick", v[0], v[1], v[2], [v[3 + 5 * k:8 + 5 * k] for k in range(v[1])]])
        elif w[0] == "sort":
            out.append(["sort", v[0], v[1], [v[2 + 4 * k:6 + 4 * k] for k in range(v[1])]])
        else:
            out.append(w)
    return out


def test_recorded_plans_replay_exactly(checker):
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "tick_plans.json")))
    names = {s["name"][0] for s in fx["scenarios"]}
    assert names == set("123456789"), names
    rows = 0
    for s in fx["scenarios"]:
        c = s["cfg"]
        ops = "cfg {n} {range_mode} {lane_tree} {quad_force} {row_max} {quad_max} {pair_max} {lane_sort_mask}\n".format(**c)
        ops += "".join(" ".join(str(x) for x in o) + "\n" for o in s["ops"])
        r = subprocess.run([checker, "replay"], input=ops, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (s["name"], r.stdout[-500:], r.stderr[-500:])
        got = _rows(r.stdout)
        assert got[0] == ["depth", str(s["depth"])], s["name"]
        assert len(got) - 1 == len(s["records"]), s["name"]
        for k, (g, w) in enumerate(zip(got[1:], s["records"])):
            assert g == w, (s["name"], k, g, w)
        rows += len(s["records"])
    assert rows >= 100


def _sweep(exe):
    r = subprocess.run([exe, "sweep"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    cases, fails = (int(x) for x in r.stdout.split("\n")[-2].split())
    assert fails == 0 and cases >= 3672, r.stdout[-3000:]   # 153 (n, L_len) x 3 modes x 2 tree forms x 4 B, + the splits
    return r


def test_planner_invariants(checker):
    _sweep(checker)


def test_planner_invariants_under_asan_ubsan(tmp_path):
    host_san = []
    for f in SAN:   # host code only: each sanitizer flag right after -Xarch_host
        host_san += ["-Xarch_host", f]
    r = _sweep(_build(tmp_path / "tpc_san", "-O1", ["-g"] + host_san))
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
