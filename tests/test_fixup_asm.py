"""The fast fix-up of csrc/field_asm.h (tools/gen_field_asm.py fix_m1 + FIX_FAST, subp_mn + SUBP_FAST)
replayed on Python integers, one lane at a time, from the emitted asm text: on every input the
emitted rare-edge test does not flag, the fast statements give the words of the exact statement
(fix_seq / the exact "+ p") of the same block.  Also: the test flags every h1 == 2^32-1 and
h4 == 2^32-1 (what the dropped h4 -> h5 link rests on), and the fix-up's VALU count."""
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "cudabulletproof_amd", "csrc", "field_asm.h")).read()
M32, M64 = 2**32 - 1, 2**64 - 1
CONST = {"c80": 0x80000000, "p0l": 0xFFFFFFED}


def _body(fn):
    b = HDR[HDR.index(f"void {fn}("):]
    return b[:b.index("\n}\n")]


def _statements(fn):
    return [[t.strip() for t in m.group(1).replace("\\n", "\n").replace("\\t", "").split("\n") if t.strip()]
            for m in re.finditer(r'asm(?: volatile)?\("((?:[^"\\]|\\.)*)"', _body(fn))]


def _calls(fn):
    """The fix-up helpers a block calls after its fast statement: [(helper, [argument names])]."""
    return [(m.group(1), [a.strip() for a in m.group(2).split(",")])
            for m in re.finditer(r"^    (fe_\w+_fast_asm)\(([^)]*)\);", _body(fn), re.M)]


def _s32(x):
    return x - 2**32 if x >> 31 else x


def run(lines, r):
    """Interpret straight-line asm on the register file r (name -> int; SGPR masks are 0 or 1)."""
    def val(tok):
        m = re.fullmatch(r"%\[(\w+)\]", tok)
        if m:
            return r[m.group(1)] if m.group(1) in r else CONST[m.group(1)]
        return int(tok, 0) & M32

    def name(tok):
        return re.fullmatch(r"%\[(\w+)\]", tok).group(1)

    for line in lines:
        op, _, rest = line.partition(" ")
        o = [x.strip() for x in rest.split(",")] if rest else []
        if op == "s_nop":
            continue
        if op in ("v_add_co_u32", "v_addc_co_u32", "v_sub_co_u32", "v_subb_co_u32"):
            c = val(o[4]) if len(o) == 5 else 0
            assert c in (0, 1)
            t = val(o[2]) + val(o[3]) + c if "add" in op else val(o[2]) - val(o[3]) - c
            r[name(o[0])], r[name(o[1])] = t & M32, int(t < 0 or t > M32)
        elif op == "v_mad_u64_u32":
            t = val(o[2]) * val(o[3]) + r[name(o[4])]
            r[name(o[0])], r[name(o[1])] = t & M64, int(t > M64)
        elif op == "v_mad_i64_i32":
            t = _s32(val(o[2])) * _s32(val(o[3])) + r[name(o[4])]
            r[name(o[0])], r[name(o[1])] = t & M64, 0   # (the carry-out is read by nothing)
        elif op == "v_add_u32":
            r[name(o[0])] = (val(o[1]) + val(o[2])) & M32
        elif op == "v_lshl_add_u32":
            r[name(o[0])] = ((val(o[1]) << val(o[2])) + val(o[3])) & M32
        elif op == "v_lshrrev_b32":
            r[name(o[0])] = val(o[2]) >> val(o[1])
        elif op == "v_ashrrev_i32":
            r[name(o[0])] = (_s32(val(o[2])) >> val(o[1])) & M32
        elif op == "v_mul_u32_u24":
            r[name(o[0])] = ((val(o[1]) & 0xFFFFFF) * (val(o[2]) & 0xFFFFFF)) & M32
        elif op == "v_cndmask_b32":
            r[name(o[0])] = val(o[2]) if val(o[3]) else val(o[1])
        elif op == "v_max_u32":
            r[name(o[0])] = max(val(o[1]), val(o[2]))
        elif op == "v_max3_u32":
            r[name(o[0])] = max(val(o[1]), val(o[2]), val(o[3]))
        elif op == "v_bfrev_b32":
            r[name(o[0])] = int(format(val(o[1]), "032b")[::-1], 2)
        elif op == "v_not_b32":
            r[name(o[0])] = val(o[1]) ^ M32
        elif op == "v_and_b32":
            r[name(o[0])] = val(o[1]) & val(o[2])
        elif op == "v_or_b32":
            r[name(o[0])] = val(o[1]) | val(o[2])
        elif op == "v_cmp_eq_u32":
            r[name(o[0])] = int(val(o[1]) == val(o[2]))
        elif op == "v_cmp_le_u32":
            r[name(o[0])] = int(val(o[1]) <= val(o[2]))
        elif op == "v_cmp_gt_i32":
            r[name(o[0])] = int(_s32(val(o[1])) > _s32(val(o[2])))
        elif op == "s_and_b64":
            r[name(o[0])] = val(o[1]) & val(o[2])
        elif op == "s_or_b64":
            r[name(o[0])] = val(o[1]) | val(o[2])
        elif op == "s_andn2_b64":
            r[name(o[0])] = val(o[1]) & (val(o[2]) ^ 1)
        elif op == "s_orn2_b64":
            r[name(o[0])] = val(o[1]) | (val(o[2]) ^ 1)
        else:
            raise AssertionError(f"opcode not modelled: {line}")
    return r


def run_helper(helper, args, r):
    """A fix-up helper's statement on the caller's words: limb 0 packed into l0 as the C glue does."""
    body = _body(helper)
    params = re.findall(r"uint32_t&? (\w+)", body[:body.index(")")])
    assert len(params) == len(args) and params[:2] == ["h0", "h1"]
    loc = {p: r[a] for p, a in zip(params, args)}
    loc["l0"] = loc["h0"] | (loc["h1"] << 32)
    (stmt,) = _statements(helper)
    run(stmt, loc)
    loc["h0"], loc["h1"] = loc["l0"] & M32, loc["l0"] >> 32
    for p, a in zip(params, args):
        if re.search(rf"uint32_t& {p}\b", body):
            r[a] = loc[p]


def words(x, n=8):
    return [(x >> (32 * i)) & M32 for i in range(n)]


def fast_and_exact(fn, a, b, outs=("h",)):
    """(srare or acc, fast words, exact words) of block fn on the operands a, b (256-bit integers)."""
    st = _statements(fn)
    regs = {f"a{i}": w for i, w in enumerate(words(a))}
    second = "x" if "fold" in fn else "b"
    regs.update({f"{second}{i}": w for i, w in enumerate(words(b))})
    f = dict(regs, acc=0)
    run(st[0], f)
    for helper, args in _calls(fn):
        run_helper(helper, args, f)
    base = fn.replace("_acc", "")
    e = run(_statements(base)[1], dict(regs))
    flag = f["srare"] if "srare" in f else int(f["acc"] == M32)
    return flag, [[f[f"{p}{i}"] for i in range(8)] for p in outs], [[e[f"{p}{i}"] for i in range(8)] for p in outs]


H0 = (0, 2**32 - 20, 2**32 - 19, 2**32 - 1)
H1 = (0, 2**32 - 2)
H4 = (0, 2**32 - 2)
H7 = (0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)


def sums(rng, h1s=H1, h4s=H4):
    """256-bit sums with the edge words of the cross product (the other words random), each with
    and without a carry out of bit 255."""
    for h0 in H0:
        for h1 in h1s:
            for h4 in h4s:
                for h7 in H7:
                    for carry in (0, 1):
                        w = [h0, h1, rng.getrandbits(32), rng.getrandbits(32), h4, rng.getrandbits(32),
                             rng.getrandbits(32), h7]
                        yield sum(x << (32 * i) for i, x in enumerate(w)), carry


def split(rng, h, carry, flagged):
    """Operands a, b with a + b = h + carry 2^256 that the block's rare-edge test does not flag."""
    for _ in range(64):
        a = rng.randrange(h + 1, 2**256) if carry else rng.randrange(0, h + 1)
        b = h + (carry << 256) - a
        if 0 <= b < 2**256 and not flagged(a, b):
            return a, b
    raise AssertionError("no unflagged split found")


ADD_FORMS = ["fe_add_asm", "fe_add_asm_lat", "fe_add_asm_lat_acc", "fe_fold_asm", "fe_fold_asm_lat", "fe_fold_asm_lat_acc"]
ADDSUB_FORMS = ["fe_addsub_asm", "fe_addsub_asm_lat", "fe_addsub_asm_lat_acc"]


@pytest.mark.parametrize("fn", ADD_FORMS + ADDSUB_FORMS)
def test_fast_fixup_matches_exact_form(fn):
    rng = random.Random(11)
    outs = ("h", "t") if "addsub" in fn else ("h",)
    cases = list(sums(rng)) + [(rng.getrandbits(256), rng.getrandbits(1)) for _ in range(400)]
    seen = set()
    for h, carry in cases:
        a, b = split(rng, h, carry, lambda a, b: fast_and_exact(fn, a, b, outs)[0])
        flag, fast, exact = fast_and_exact(fn, a, b, outs)
        assert flag == 0
        assert fast[0] == exact[0], (fn, hex(a), hex(b))
        assert fast == exact, (fn, hex(a), hex(b))
        seen.add((carry, h >> 255))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_fast_sub_matches_exact_form():
    """fe_sub_asm's fast "+ p" (one 64-bit multiply-add on limb 0): t0's low word around 19, t1 != 0
    (t0 < 19 is a rare edge), bit 255 either way, with and without a final borrow."""
    rng = random.Random(12)
    cases = []
    for t0 in (0, 18, 19, 2**32 - 1):
        for t1 in (1, 2**32 - 1):
            for t7 in H7:
                for borrow in (0, 1):
                    w = [t0, t1] + [rng.getrandbits(32) for _ in range(5)] + [t7]
                    cases.append((sum(x << (32 * i) for i, x in enumerate(w)), borrow))
    cases += [(rng.getrandbits(256), rng.getrandbits(1)) for _ in range(400)]
    for t, borrow in cases:
        for _ in range(64):   # a - b = t - borrow 2^256
            b = rng.randrange(2**256 - t, 2**256) if borrow else rng.randrange(0, 2**256 - t)
            a = t + b - (borrow << 256)
            if 0 <= a < 2**256 and not fast_and_exact("fe_sub_asm", a, b)[0]:
                break
        else:
            raise AssertionError("no unflagged operands found")
        flag, fast, exact = fast_and_exact("fe_sub_asm", a, b)
        assert flag == 0 and fast == exact, (hex(a), hex(b))


@pytest.mark.parametrize("fn", ADD_FORMS + ADDSUB_FORMS)
def test_rare_edge_test_flags_h1_and_h4_all_ones(fn):
    """With h4 == 2^32-1 excluded, h4 + m cannot carry into h5: the fast fix-up has no such link."""
    rng = random.Random(13)
    outs = ("h", "t") if "addsub" in fn else ("h",)
    n = 0
    for h1s, h4s in (((M32,), H4 + (M32,)), (H1 + (M32,), (M32,))):
        for h, carry in sums(rng, h1s, h4s):
            a = rng.randrange(h + 1, 2**256) if carry else rng.randrange(0, h + 1)
            b = h + (carry << 256) - a
            if not 0 <= b < 2**256:
                continue
            assert fast_and_exact(fn, a, b, outs)[0] == 1, (fn, hex(a), hex(b))
            n += 1
    assert n == 2 * 96


def _is_valu(line):
    return line.startswith("v_")


@pytest.mark.parametrize("fn,chain_end,limit", [(f, r"v_addc_co_u32 %\[h7\]", 5) for f in ADD_FORMS] +
                         [(f, r"v_subb_co_u32 %\[t7\]", 5 + 3) for f in ADDSUB_FORMS] +
                         [("fe_sub_asm", r"v_subb_co_u32 %\[h7\]", 3)])
def test_fast_fixup_valu_count(fn, chain_end, limit):
    """Everything a fast form issues after its carry chain's last link: m1 (two VALU) and the three
    additions of the fix-up; add/sub's also holds sub's mn and its two additions."""
    fast = _statements(fn)[0]
    last = max(i for i, t in enumerate(fast) if re.match(chain_end, t))
    tail = [t for t in fast[last + 1:] if _is_valu(t)]
    helpers = [t for h, _ in _calls(fn) for t in _statements(h)[0]]
    assert all(_is_valu(t) for t in helpers)
    assert len(tail) + len(helpers) <= limit, (tail, helpers)
    assert not any("c80" in t for t in fast + helpers)   # no 0x80000000 operand to materialise


def test_canon_fast_path_matches_exact_path():
    """fe_canon_asm (fe_mul_one): one statement, the fast and the exact path either side of the
    wave-uniform branch; the fast path (32-bit words, no h5 link) against the exact one."""
    (st,) = _statements("fe_canon_asm")
    br, jmp, slow, end = st.index("s_cbranch_scc1 3f"), st.index("s_branch 4f"), st.index("3:"), st.index("4:")
    pre, fast, exact = st[:br - 1], st[br + 1:jmp], st[slow + 1:end]
    assert st[br - 1].startswith("s_cmp_lg_u64 %[srare]")
    assert sum(_is_valu(t) for t in fast) <= 6
    rng = random.Random(14)
    n = 0
    for h, _ in list(sums(rng)) + [(rng.getrandbits(256), 0) for _ in range(300)]:
        regs = run(pre, {f"h{i}": w for i, w in enumerate(words(h))})
        if regs["srare"]:
            continue
        f, e = run(fast, dict(regs)), run(exact, dict(regs))
        assert [f[f"h{i}"] for i in range(8)] == [e[f"h{i}"] for i in range(8)], hex(h)
        n += 1
    assert n > 300
    for h, _ in sums(rng, (M32,), H4 + (M32,)):
        assert run(pre, {f"h{i}": w for i, w in enumerate(words(h))})["srare"] == 1
