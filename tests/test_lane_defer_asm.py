"""The lane loops' deferred rare-edge and gate tests (ge25519_dev.h: the point forms in the Defer
mode; fe25519_dev.h LAT 3), checked on the CPU from the emitted text.

* field_asm.h's throughput *_acc statements are their split block's fast statement with the one
  rare-edge compare replaced by the running max into acc: the same instructions otherwise.
* Replayed on Python integers over the fix-up's edge word patterns (tests/test_fixup_asm.py): a lane
  reaches acc == 2^32-1 exactly when the split form sets srare for it, whatever acc held before (as
  long as it was not already 2^32-1: the word is sticky), and its words are the fast statement's.
* The product gate's deferred form (fe25519_dev.h mul_gate_defer, one v_max3_u32) leaves gacc above
  MUL_BOUNDED_WORD exactly when max(a0, b7) is, or gacc already was.
"""
import os
import random
import re

import pytest

from test_fixup_asm import HDR, M32, _calls, _statements, fast_and_exact, run, run_helper, sums, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudabulletproof_amd", "csrc")
FORMS = ["fe_add_asm", "fe_sub_asm", "fe_fold_asm", "fe_addsub_asm"]
CMP, MAX = "v_cmp_eq_u32 %[srare], -1, %[vt3]", "v_max_u32 %[acc], %[acc], %[vt3]"


def _raw_statements(fn):
    body = HDR[HDR.index(f"void {fn}("):]
    body = body[:body.index("\n}\n")]
    return [m.group(1) for m in re.finditer(r'asm volatile\("((?:[^"\\]|\\.)*)"', body)]


@pytest.mark.parametrize("fn", FORMS)
def test_acc_statements_are_the_fast_statements(fn):
    fast = _raw_statements(fn)[0]
    acc = _raw_statements(fn + "_acc")
    assert len(acc) == 1 and fast.count(CMP) == 1
    assert acc[0] == fast.replace(CMP, MAX)
    # no SALU test, no branch, and the same fast fix-up calls after the statement
    assert not re.search(r"s_cmp|s_cbranch|s_branch", acc[0])
    assert _calls(fn + "_acc") == _calls(fn)
    body = HDR[HDR.index(f"void {fn}_acc("):]
    assert "srare" not in body[:body.index("\n}\n")]


def _acc_run(fn, a, b, acc0, outs):
    """The _acc block on (a, b) with the running word acc0: (acc after, words)."""
    second = "x" if "fold" in fn else "b"
    r = {f"a{i}": w for i, w in enumerate(words(a))}
    r.update({f"{second}{i}": w for i, w in enumerate(words(b))})
    r["acc"] = acc0
    run(_statements(fn + "_acc")[0], r)
    for helper, args in _calls(fn + "_acc"):
        run_helper(helper, args, r)
    return r["acc"], [[r[f"{p}{i}"] for i in range(8)] for p in outs]


def _split_fast(fn, a, b, outs):
    """The split block's fast statement + fix-up on (a, b): (srare, words)."""
    second = "x" if "fold" in fn else "b"
    r = {f"a{i}": w for i, w in enumerate(words(a))}
    r.update({f"{second}{i}": w for i, w in enumerate(words(b))})
    run(_statements(fn)[0], r)
    for helper, args in _calls(fn):
        run_helper(helper, args, r)
    return r["srare"], [[r[f"{p}{i}"] for i in range(8)] for p in outs]


@pytest.mark.parametrize("fn", FORMS)
def test_acc_saturates_exactly_when_srare(fn):
    rng = random.Random(21 + FORMS.index(fn))
    outs = ("h", "t") if "addsub" in fn else ("h",)
    edge = (0, 2**32 - 2, M32)
    cases = list(sums(rng, edge, edge)) + [(rng.getrandbits(256), rng.getrandbits(1)) for _ in range(300)]
    flagged = clear = 0
    for h, carry in cases:
        if fn == "fe_sub_asm":   # a - b = h - carry 2^256
            b = rng.randrange(2**256 - h, 2**256) if carry else rng.randrange(0, 2**256 - h)
            a = h + b - (carry << 256)
        else:                    # a + b = h + carry 2^256
            a = rng.randrange(h + 1, 2**256) if carry else rng.randrange(0, h + 1)
            b = h + (carry << 256) - a
        if not (0 <= a < 2**256 and 0 <= b < 2**256):
            continue
        if rng.random() < 0.2:   # the operand-side tests (sub's and fold's x / g words)
            b |= M32 << (32 * rng.choice((2, 4, 6)))
        srare, fast = _split_fast(fn, a, b, outs)
        for acc0 in (0, rng.getrandbits(32) % M32, M32 - 1):
            acc, got = _acc_run(fn, a, b, acc0, outs)
            assert (acc == M32) == bool(srare), (fn, hex(a), hex(b), hex(acc0))
            assert acc >= acc0 and got == fast
        assert _acc_run(fn, a, b, M32, outs)[0] == M32   # sticky
        if not srare:            # and the words are then the exact form's (the split form's own contract)
            flag, f2, exact = fast_and_exact(fn, a, b, outs)
            assert flag == 0 and f2 == exact == fast
        flagged += bool(srare)
        clear += not srare
    assert flagged > 50 and clear > 300, (flagged, clear)


def _gate_asm():
    src = open(os.path.join(CSRC, "fe25519_dev.h")).read()
    body = src[src.index("void mul_gate_defer("):]
    body = body[:body.index("\n}\n")]
    (text,) = re.findall(r'asm\("([^"]*)"', body)
    return text, src


def test_gate_word_exceeds_bound_exactly_when_the_gate_fails():
    text, src = _gate_asm()
    assert text == "v_max3_u32 %0, %0, %1, %2"
    line = text.replace("%0", "%[gacc]").replace("%1", "%[x]").replace("%2", "%[y]")
    bound = int(re.search(r"MUL_BOUNDED_WORD = 0x([0-9A-F]+)u", open(os.path.join(CSRC, "mul512_asm.h")).read()).group(1), 16)
    assert bound == 0xFFFFFFEF
    rng = random.Random(31)
    vals = (0, 1, bound - 1, bound, bound + 1, 0xFFFFFFF0, M32)
    n = 0
    for a0 in vals + tuple(rng.getrandbits(32) for _ in range(20)):
        for b7 in vals + tuple(rng.getrandbits(32) for _ in range(20)):
            for g0 in (0, bound, bound + 1, rng.getrandbits(32)):
                g = run([line], {"gacc": g0, "x": a0, "y": b7})["gacc"]
                assert (g > bound) == (max(a0, b7) > bound or g0 > bound), (hex(a0), hex(b7), hex(g0))
                assert g >= g0
                n += 1
    assert n == 27 * 27 * 4
    # the deferred product paths: the bounded form, the gate's words into gacc, no vote and no branch;
    # mul512 gates on (a[0], b[7]), sqr512 on (a[0], a[7]), the same words as the inline gates
    for fn, words_, bounded in (("mul512", "a[0], b[7]", "mul512_bounded_asm(w, a, b);"),
                                ("sqr512", "a[0], a[7]", "sqr512_offdiag_bounded_asm(o, a);")):
        body = src[src.index(f"BP_DEV void {fn}("):]
        body = body[:body.index("\n#else")]
        i = body.index(bounded)
        nxt = body[i + len(bounded):].strip().splitlines()
        assert nxt[0].strip() == f"if constexpr (DEFER) mul_gate_defer(*gacc, {words_});"
        assert nxt[1].strip().startswith(f"else if (__builtin_expect(__any(max({words_}) > MUL_BOUNDED_WORD), 0))")


def _body(src, head):
    body = src[src.index(head):]
    return body[:body.index("\n}\n")]


def test_loops_run_the_deferred_forms_and_rerun_on_a_hit():
    """ge25519_dev.h: the point forms reach their field blocks only through the mode's forwards, whose
    Defer mode is LAT 3 with both running words and whose Gated mode is LAT 0 (fe_mul_one keeps its own
    test), the two loops' deferred instantiation tests the running words once per chunk and once after
    the loop and warms up with the gated overload, and scalarmult / sm_lane fall through to the gated
    instantiation when the deferred pass reports a hit."""
    src = open(os.path.join(CSRC, "ge25519_dev.h")).read()
    # (a) no point form calls a field block with a literal mode
    field = r"\bfe_(?:add|sub|mul|sq|mul_k|addsub)\b"
    for head in ("BP_DEV ge ge_tail(", "BP_DEV ge ge_dbl(const ge& p, M& m)", "BP_DEV ge ge_add_qp(const ge& p, const geq* q, bool zone, M& m)",
                 "BP_DEV ge ge_add_sel(const ge& p, const geq* q, bool use_q, M& m)"):
        body = _body(src, head)
        assert re.findall(r"\bm_(?:add|sub|mul|sq|mul_k|addsub)\(", body) and not re.findall(field, body), head
    assert len(re.findall(r"\bBP_DEV ge (?:ge_tail|ge_dbl|ge_add_qp|ge_add_sel)\(", src)) == 7   # + the three gated overloads
    assert not re.search(r"\b\w+_d\b\s*[<(]", src)                                             # no second family
    forwards = {m.group(1): m.group(2) for m in re.finditer(r"BP_DEV \w+ m_(\w+)\(.*?\) \{(.*?)\n?\}\n", src, re.S)}
    assert sorted(forwards) == ["add", "addsub", "mul", "mul_k", "sq", "sub"]
    for name, body in forwards.items():
        calls = re.findall(r"\b(fe_\w+)<([^>]*)>\(([^;]*)\);", body)
        assert calls and all(t == "M::LAT" and "m.edge()" in args for _, t, args in calls), (name, calls)
        assert all(("m.gate()" in args) == (fn in ("fe_mul", "fe_sq")) for fn, _, args in calls), (name, calls)
    assert {fn for fn, _, _ in re.findall(r"\b(fe_\w+)<([^>]*)>\(([^;]*)\);", forwards["addsub"])} == {"fe_addsub", "fe_sub", "fe_add"}
    gated, defer = _body(src, "struct Gated {"), _body(src, "struct Defer {")
    assert "LAT = 0;" in gated and gated.count("return nullptr;") == 2
    assert "LAT = 3;" in defer and "edge() { return &acc; }" in defer and "gate() { return &gacc; }" in defer
    # (b), (c) each loop: two tests of the running words in the deferred instantiation only, the warm-up gated
    for head, warm in (("BP_DEV bool sm_uniform(", "r = ge_dbl(r);"), ("BP_DEV bool sm_lane_loop(", "r = ge_add_sel<QLDS, ZONE>(r, q, add_phase);")):
        body = _body(src, head)
        tests = [l.strip() for l in body.splitlines() if "defer_hit(m)" in l]
        assert len(tests) == 2 and body.count("defer_hit(") == 2 and "BP_DEFER_CHUNK" in body
        assert "std::conditional_t<DEFER, Defer, Gated> m;" in body
        chunk = body[body.index("if (DEFER && ++n == BP_DEFER_CHUNK) {"):]
        assert tests[0] in chunk[:chunk.index("\n        }\n")] and tests[1].startswith("if (DEFER && ")
        w = body.index(warm)
        assert "DEFER" in body[:w].splitlines()[-1] + body[:w].splitlines()[-2] and w < body.index("conditional_t")
    assert "ge_add_qp<QLDS>(r, q, zone);" in _body(src, "BP_DEV bool sm_uniform(").split("conditional_t")[0]
    # (d) the gated instantiation after a deferred pass that returned false
    sm = src[src.index("BP_DEV ge scalarmult("):]
    assert re.search(r"#if BP_LANE_DEFER\s*if \(sm_uniform<QLDS, true, FORCE>\(r, s, q, dtab, ptab, K\)\) return r;\s*#endif\s*"
                     r"sm_uniform<QLDS, false>\(r, s, q, dtab, ptab, K\);\s*return r;", sm)
    lane = _body(src, "BP_DEV ge sm_lane(")
    assert re.search(r"#if BP_LANE_DEFER\s*if \(zone \? sm_lane_loop<QLDS, true, true, FORCE>\(r, s, q, dtab, ptab, K\)\s*"
                     r": sm_lane_loop<QLDS, false, true, FORCE>\(r, s, q, dtab, ptab, K\)\)\s*return r;\s*#endif\s*"
                     r"if \(zone\) sm_lane_loop<QLDS, true, false>\(r, s, q, dtab, ptab, K\);\s*"
                     r"else sm_lane_loop<QLDS, false, false>\(r, s, q, dtab, ptab, K\);\s*return r;", lane)
