"""The host provers' plan and result owner (csrc/bp_host_prove.h: how
hipbp_batch_generate_range_proof_host_sharded and hipbp_batch_generate_range_proof_accepted_host cut a
call into shards and chunks, and how a failed call frees and zeroes what its shards handed out) run on
the CPU by tests/host_prove_check.hip, a stand-alone host program:

* the plan over count in {1, 2, 3, 9, 70, 65537}, ng in {1, 2, 3, 8, 64}, chunk in {1, 4, 16384},
  index_base in {0, 2^32 - 3, 2^64 - 2}: the shards are contiguous and disjoint, cover [0, count) and
  differ in size by at most 1, none is empty when ng <= count; every shard's chunks cover it in order,
  every chunk's base is index_base + c0 mod 2^64, and the wrap is reached.
* the owner: 9 proofs (L_len 0 and 4, proof 5 refused, with and without attempts) filled from three
  threads and rolled back: no vector is left, every struct, valid and attempts byte is zero; the same
  with the k-th allocation failing for every k up to the total (32) and one past it.

Once at -O2 and once under AddressSanitizer + UndefinedBehaviourSanitizer (host code only, nothing
loaded into Python).  A device failure is never provoked on a GPU to test the rollback: this is
its test."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_prove_check.hip")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")


def _build(exe, opt, extra=()):
    subprocess.run(["hipcc", opt, "-std=c++17", "--cuda-host-only", "-x", "hip", SRC, "-o", str(exe), "-pthread"] + list(extra),
                   check=True, capture_output=True)
    return str(exe)


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    checks, fails = (int(x) for x in r.stdout.split("\n")[-2].split())
    # 270 plans of at least 4 checks and, at count = 65537 and chunk = 1, 3 per chunk (15 plans of 65537
    # chunks); 136 owner cases of at least 6; 937 checks of the shard count and 76 of the fan-out
    assert fails == 0 and checks >= 270 * 4 + 15 * 65537 * 3 + 136 * 6 + 937 + 76, r.stdout[-3000:]
    return r


def test_plan_and_owner(tmp_path):
    _run(_build(tmp_path / "hp", "-O2"))


def test_plan_and_owner_under_asan_ubsan(tmp_path):
    host_san = []
    for f in SAN:   # host code only: each sanitizer flag right after -Xarch_host
        host_san += ["-Xarch_host", f]
    r = _run(_build(tmp_path / "hp_san", "-O1", ["-g"] + host_san))
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
