"""The voted per-lane step's agreeing paths in the compiler's output (CPU only: tools/isa_count.py compiles
tools/isa_ops.hip for gfx950 and counts ordinary opcodes per probe kernel).

With the vote forced to "all lanes doubling" or "all lanes adding", ge_add_sel must be the pure form: no
per-lane operand select and exactly the pure form's products.  The forced "mixed" path must be today's
selected step, and the voting probe must hold the three stage-1 bodies and one tail, not three steps.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")


@pytest.fixture(scope="module")
def counts():
    """probe kernel -> {VALU opcode: count} (the common path, as tools/isa_count.py reports it)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_count.py")], check=True, text=True,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ISA_FULL="p_")).stdout
    res, name = {}, None
    for line in out.splitlines():
        m = re.match(r"^(p_\w+)(?: \(loop body\))?\s+VALU\s+(\d+)", line)
        if m:
            name = m.group(1)
            res[name] = {"VALU": int(m.group(2))}
        elif line.startswith("    ") and name:
            for tok in line.strip().split(", "):
                op, _, n = tok.rpartition(":")
                res[name][op] = int(n)
    return res


def _selects(c):
    return c.get("v_cndmask_b32_e32", 0)


def test_agreeing_paths_are_the_pure_forms(counts):
    dbl, add = counts["p_ge_add_vote_zone_d_dbl"], counts["p_ge_add_vote_zone_d_add"]
    assert _selects(counts["p_ge_add_sel_zone_d"]) >= 24      # what the selected step pays: three operands and ZZ
    assert _selects(dbl) == 0 and _selects(add) == 0
    assert dbl["v_mad_u64_u32"] == counts["p_ge_dbl_d"]["v_mad_u64_u32"]
    assert add["v_mad_u64_u32"] == counts["p_ge_add_zone_d"]["v_mad_u64_u32"]
    assert dbl["VALU"] <= counts["p_ge_dbl_d"]["VALU"] and add["VALU"] <= counts["p_ge_add_zone_d"]["VALU"]


def test_mixed_path_is_the_selected_step(counts):
    sel = counts["p_ge_add_vote_zone_d_sel"]
    assert sel["v_mad_u64_u32"] == counts["p_ge_add_sel_zone_d"]["v_mad_u64_u32"]
    assert sel["VALU"] <= counts["p_ge_add_sel_zone_d"]["VALU"]


def test_one_tail_for_the_three_bodies(counts):
    """The voting probe holds the three stage-1 bodies and one tail: its products are the three forced
    paths' minus two tails, a tail being four general products (p_fe_mul each) and three add / sub blocks
    (at most one multiply-add each, the fix-up's)."""
    three = sum(counts["p_ge_add_vote_zone_d" + s]["v_mad_u64_u32"] for s in ("_dbl", "_add", "_sel"))
    twice_tail = three - counts["p_ge_add_vote_zone_d"]["v_mad_u64_u32"]
    mul = counts["p_fe_mul"]["v_mad_u64_u32"]
    assert twice_tail % 2 == 0 and 4 * mul <= twice_tail // 2 <= 4 * mul + 3
