"""The flat batch layouts and workspace tables (csrc/bp_layout.h: the verify chunk, the proof output,
the proof vectors, every workspace buffer's size) run on the CPU by tests/layout_check.hip, a
stand-alone host program:

* offsets: over c in {1, 2, 3, 1024}, ab_len in {1, 2, 3}, L_len in {0, 1, 6, 16} (and cap in
  {c, c + 1, 16384} for the proof output) every region lies where the formulas the library used
  before the layouts had one definition put it; the regions are in order, disjoint and 32-byte aligned.
* pack / view and output / unpack round trips with distinct bytes in every field, with and without
  the range-proof part, with refused proofs, at L_len = 0 and with a short last chunk.
* every buffer of the prover, IPA, MSM and verify-slot tables has its listed size.
* the Pippenger part: over n in {1, 3, 4, 63, 64, 1000, 3000, 65536, 2^20}, c in {4, 8, 12}, count in
  {1, 3}, the window ranges [0, W), [0, 1), [wm, W), both key widths and tail layers {1, 4, 8}, every
  field of pip_shape and every buffer's bytes equal the expressions bp_pippenger.hip computed in line
  before it had a table; the grid reaches both key widths, a part with and without the LDS tail,
  n % 4 != 0, n < 2^c / 4 and a bidfill queue of one entry.
* the generator view: for n in {1, 2, 4} pack_gens followed by GenView::at gives back G, H, g and h,
  position k of the packed buffer is base k of the prefix-table order (G | H | h | g), a set without
  g is its first 2n + 1 points, and a view's table is null exactly when its bits are 0.

Once at -O2 and once under AddressSanitizer + UndefinedBehaviourSanitizer (host code only, nothing
loaded into Python): the round trips use exactly sized buffers and free every vector handed out."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "layout_check.hip")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")


def _build(exe, opt, extra=()):
    subprocess.run(["hipcc", opt, "-std=c++17", "--cuda-host-only", "-x", "hip", SRC, "-o", str(exe)] + list(extra),
                   check=True, capture_output=True)
    return str(exe)


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    checks, fails = (int(x) for x in r.stdout.split("\n")[-2].split())
    # 48 chunk shapes and 96 output shapes of >= 12 regions, 72 round trips, 12 unpack shapes, the tables
    # (5000 at least), and 40 checks for each of the Pippenger grid's 972 shapes + 3 for its coverage
    assert fails == 0 and checks >= 5000 + 972 * 40 + 3, r.stdout[-3000:]
    return r


def test_layouts_and_tables(tmp_path):
    _run(_build(tmp_path / "lc", "-O2"))


def test_layouts_and_tables_under_asan_ubsan(tmp_path):
    host_san = []
    for f in SAN:   # host code only: each sanitizer flag right after -Xarch_host
        host_san += ["-Xarch_host", f]
    r = _run(_build(tmp_path / "lc_san", "-O1", ["-g"] + host_san))
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
