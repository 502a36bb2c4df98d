"""The verify pipeline's tick planner (csrc/bp_tick_plan.h: the stage table, plan_tick, lane_sort_sets)
run on the CPU by tests/tick_plan_check.hip, a stand-alone host program:

* replay: every scenario of tests/golden/tick_plans.json (the plans the library launched before the
  planner was split out of Pipeline::push; tests/golden/tick_plans.README.md) gives the recorded
  rows exactly: tick form, region count, total and every region's (kind, slot, r, begin, items);
  the lane sort's sets and blocks; the pipeline depth.
* sweep: the planner's invariants over n = 1 .. 65536, every mode, L_len, tree form, split stage 0
  where it applies, B in {1, 63, 64, 1000}, full and draining pipelines; then free-form rings, every
  push with its own B, L_len and split flag and drain ticks mixed in (descending, ascending, sawtooth,
  constant and 2000 seeded random sequences per n, mode and tree form), under the admission contract
  of Pipeline::push (push_admits): an accepted push is followed only by ticks that plan, a refused
  one leaves the ring byte-identical and is accepted after at most `depth` drain ticks, a uniform
  ring is never refused, and the descending-round sequences are refused exactly where the region
  list would overflow; once more under AddressSanitizer + UndefinedBehaviourSanitizer (host code
  only, nothing loaded into Python; 100 random sequences per configuration there).
* the refusal as the library's caller meets it (replay), the push it falls on, and the tick that
  retires a batch (tests/pipeline_seq.py retire_tick, which the GPU sequence tests rely on)."""
import json
import os
import shutil
import subprocess

import pytest

from pipeline_seq import REFUSED_PUSH, descending_ops, retire_tick

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


def _sweep(exe, random_per_cfg=2000):
    r = subprocess.run([exe, "sweep", str(random_per_cfg)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    cases, fails = (int(x) for x in r.stdout.split("\n")[-2].split())
    assert fails == 0 and cases >= 3672, r.stdout[-3000:]   # 153 (n, L_len) x 3 modes x 2 tree forms x 4 B, + the splits
    free = int(r.stdout.split("\n")[-3].split()[-1])
    print(f"free-form rings: {free}, failures: {fails}")
    # 7 n x 3 modes x 2 tree forms: the random sequences, and 3 split patterns x 6 B x (3 + log2 n + 1) structured
    assert free >= 42 * random_per_cfg + 3 * 6 * 3 * 42, r.stdout[-3000:]
    for n, mode in ((2048, 2), (4096, 2), (65536, 2)):   # the default configuration's refusals, as printed
        assert f"descending n {n} mode {mode} raised 0 defer 0: refused 1" in r.stdout
    assert "descending n 1024 mode 2 raised 0 defer 0: refused 0" in r.stdout
    return r


def test_planner_invariants(checker):
    _sweep(checker)


def test_planner_invariants_under_asan_ubsan(tmp_path):
    host_san = []
    for f in SAN:   # host code only: each sanitizer flag right after -Xarch_host
        host_san += ["-Xarch_host", f]
    r = _sweep(_build(tmp_path / "tpc_san", "-O1", ["-g"] + host_san), 100)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


DEFAULT_CFG = "cfg {n} {mode} {lane_tree} -1 2048 16384 32768 7\n"


def _replay(checker, n, mode, lane_tree, ops):
    """ops as tests/pipeline_seq.py writes them (B, L_len of each push; `defer` the split flag from then on)
    -> (rows, per accepted push its own tick's index, indices of the refused pushes)."""
    text, split = DEFAULT_CFG.format(n=n, mode=mode, lane_tree=int(lane_tree)), 0
    for op in ops:
        if op[0] == "defer":
            split = int(op[1])
        else:
            text += f"push {op[1]} {op[2]} {split}\n" if op[0] == "push" else op[0] + "\n"
    r = subprocess.run([checker, "replay"], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    rows = _rows(r.stdout)[1:]
    ticks = [w for w in rows if w[0] == "tick"]
    pushed, refused, t = [], [], 0
    for w in rows:
        if w[0] == "sort":
            pushed.append(t)
        elif w[0] == "refused":
            refused.append(len(pushed) + len(refused))
        elif w[0] == "tick":
            t += 1
    return ticks, pushed, refused, int(_rows(r.stdout)[0][1])


RK_FINAL = 4


def _final_ticks(ticks, pushed, depth):
    """For each accepted push the index of the tick that holds its RK_FINAL region."""
    out = []
    for t0 in pushed:
        hits = [t for t in range(t0, min(t0 + depth, len(ticks)))
                if any(g[0] == RK_FINAL and g[1] == t0 % depth for g in ticks[t][4])]
        assert len(hits) == 1, (t0, hits)
        out.append(hits[0])
    return out


def test_descending_rounds_are_refused_and_the_ring_goes_on(checker):
    """Round counts 11 .. 2 at n = 2048, mode 2, then full-L batches: every batch reaches its final-terms
    stage in one tick, whose region list cannot hold the 13th batch's regions too.  That push is
    refused with nothing staged; after one drain tick the same batch is accepted, and every batch
    (the 12 in flight at the refusal included) runs each of its stages and retires."""
    ops = [("push", 2, L) for L in range(11, 1, -1)] + [("push", 2, 11)] * 3 + [("tick",), ("push", 2, 11), ("flush",)]
    ticks, pushed, refused, depth = _replay(checker, 2048, 2, 0, ops)
    assert refused == [12] and len(pushed) == 13
    assert pushed == list(range(12)) + [13]          # no tick ran for the refused push
    fins = _final_ticks(ticks, pushed, depth)
    want = [t0 + retire_tick(2, L) for t0, L in zip(pushed, list(range(11, 1, -1)) + [11] * 3)]
    assert fins == want and len(ticks) == max(want) + 1
    assert max(t[2] for t in ticks) <= 24


@pytest.mark.parametrize("n,mode,split", sorted(REFUSED_PUSH))
def test_refused_push_of_the_descending_sequences(checker, n, mode, split):
    """The push the GPU refusal tests expect to be refused, and the drain ticks after which the same
    batch is accepted: not one fewer (tests/pipeline_seq.py REFUSED_PUSH)."""
    at, drain = REFUSED_PUSH[(n, mode, split)]
    ops = [("defer", split)] + descending_ops(n)[:at + 1]
    for ticks, want in ((drain, [at]), (drain - 1, [at, at + 1])):
        seq = ops + [("tick",)] * ticks + ops[-1:] + [("flush",)]
        _, pushed, refused, depth = _replay(checker, n, mode, split or n <= 64, seq)
        assert refused == want and drain <= depth, (ticks, refused)


def test_retire_tick_formula(checker):
    """A batch's outputs are complete after retire_tick(mode, L_len) further ticks: the formula the GPU
    sequence tests wait by equals the planner's RK_FINAL tick for every (mode, L_len), alone in the
    ring, in both tree forms, and among batches of other round counts with drain ticks between."""
    for mode in range(3):
        for L in range(17):
            ft = L + 1 if L else 1
            last = ft
            if mode != 0:
                last = max(last, 2)
            if mode == 2:
                last = max(last, max(ft, 3))
            assert retire_tick(mode, L) == last + 1
            for lane_tree in (0, 1):
                ticks, pushed, refused, depth = _replay(checker, 65536, mode, lane_tree, [("push", 3, L), ("flush",)])
                assert not refused and _final_ticks(ticks, pushed, depth) == [retire_tick(mode, L)], (mode, L, lane_tree)
        Ls = [4, 3, 2, 1, 0, 0, 1, 2, 3, 4, 4, 0, 3, 1, 2]
        ops = []
        for k, L in enumerate(Ls):
            ops += [("push", 3 + k, L)] + [("tick",)] * (k % 3 == 2)
        ticks, pushed, refused, depth = _replay(checker, 16, mode, 1, ops + [("flush",)])
        assert not refused
        assert _final_ticks(ticks, pushed, depth) == [t0 + retire_tick(mode, L) for t0, L in zip(pushed, Ls)]
