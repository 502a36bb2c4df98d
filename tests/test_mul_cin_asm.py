"""The *_cin_asm products of csrc/mul512_asm.h (tools/gen_mul_asm.py split_cin: a column that follows one
with no counted carry reads its carry-in as an operand of its own and writes a fresh accumulator)
replayed on Python integers from the emitted text, C glue between the statements included: the same
words as the in-place forms on every input (gate words above the bound too, where neither is the
product), the exact product wherever the gate words are within the bound, and the same instructions
but for the one operand.  Also: the glue in fe25519_dev.h / ge25519_dev.h gates the new forms on the
same words and falls back to the same counting forms."""
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudabulletproof_amd", "csrc")
HDR = open(os.path.join(CSRC, "mul512_asm.h")).read()
M32, M64 = 2**32 - 1, 2**64 - 1
BOUND = int(re.search(r"MUL_BOUNDED_WORD = 0x([0-9A-F]+)u", HDR).group(1), 16)
PAIRS = [("mul512_bounded_asm", "mul512_bounded_cin_asm"),
         ("sqr512_offdiag_bounded_asm", "sqr512_offdiag_bounded_cin_asm"),
         ("mul512_k_asm", "mul512_k_cin_asm")]


def _body(fn):
    b = HDR[HDR.index(f"void {fn}("):]
    return b[:b.index("\n}\n")]


def _steps(fn):
    """The function body as a list of steps: ("asm", [instruction lines]) or ("c", statement)."""
    body = _body(fn)
    body = body[body.index("{") + 1:]
    steps, pos = [], 0
    for m in re.finditer(r'asm volatile\("((?:[^"\\]|\\.)*)"[^;]*;', body):
        steps += [("c", c.strip()) for c in body[pos:m.start()].split(";") if c.strip()]
        steps.append(("asm", [t.strip() for t in m.group(1).replace("\\n", "\n").replace("\\t", "").split("\n") if t.strip()]))
        pos = m.end()
    steps += [("c", c.strip()) for c in body[pos:].split(";") if c.strip()]
    return steps


def _kw(fn):
    m = re.search(r"kw\[8\] = \{([^}]*)\}", _body(fn))
    return [int(x.replace("u", ""), 16) for x in m.group(1).split(",")] if m else None


def replay(fn, a, b=None):
    """The function's output words on the operand words a (and b), every statement interpreted."""
    r = {f"a{i}": x for i, x in enumerate(a)}
    kw = _kw(fn)
    for j, x in enumerate(kw if kw else (b if b is not None else a)):
        r[f"b{j}"] = x
    r["acc"], out = 0, {}

    def val(tok):
        m = re.fullmatch(r"%\[(\w+)\]", tok)
        return r[m.group(1)] if m else int(tok, 0)

    for kind, s in _steps(fn):
        if kind == "asm":
            for line in s:
                op, _, rest = line.partition(" ")
                o = [x.strip() for x in rest.split(",")]
                if op == "s_nop":
                    continue
                d, sd = o[0][2:-1], o[1][2:-1]
                if op == "v_mad_u64_u32":
                    t = val(o[2]) * val(o[3]) + val(o[4])
                    r[d], r[sd] = t & M64, int(t > M64)
                elif op == "v_addc_co_u32":
                    t = val(o[2]) + val(o[3]) + val(o[4])
                    assert t <= M32
                    r[d], r[sd] = t, 0
                else:
                    raise AssertionError(f"opcode not modelled: {line}")
        elif re.fullmatch(r"uint(64|32)_t .*|constexpr .*|\(void\).*", s):
            continue
        elif s == "cin = acc >> 32":
            r["cin"] = r["acc"] >> 32
        elif s == "acc >>= 32":
            r["acc"] >>= 32
        elif s == "acc = (acc >> 32) | ((uint64_t)c2 << 32)":
            r["acc"] = (r["acc"] >> 32) | (r["c2"] << 32)
        else:
            m = re.fullmatch(r"[wo]\[(\d+)\] = (.*)", s)
            assert m, s
            out[int(m.group(1))] = {"0": 0, "(uint32_t)acc": r["acc"] & M32,
                                    "(uint32_t)(acc >> 32)": (r["acc"] >> 32) & M32}[m.group(2)]
    assert sorted(out) == list(range(16))
    return [out[k] for k in range(16)]


def _int(w):
    return sum(x << (32 * i) for i, x in enumerate(w))


def _operands(rng):
    """Word lists: zero, all ones within the gate, the gate words at, below and above the bound, random."""
    edge = [[0] * 8, [M32] * 8, [BOUND] * 8, [BOUND] + [M32] * 6 + [BOUND]]
    for g in (BOUND - 1, BOUND, BOUND + 1, M32):
        edge.append([g] + [rng.getrandbits(32) for _ in range(6)] + [g])
        edge.append([g] + [M32] * 6 + [g])
    return edge + [[rng.getrandbits(32) for _ in range(8)] for _ in range(150)]


@pytest.mark.parametrize("base,cin", PAIRS)
def test_cin_form_gives_the_in_place_forms_words_and_the_exact_product(base, cin):
    rng = random.Random(41)
    ops = _operands(rng)
    kw = _kw(cin)
    n_exact = n_over = 0
    for a in ops:
        for b in ([None] if "sqr" in cin or kw else ops[:12] + ops[-3:]):
            got = replay(cin, a, b)
            assert got == replay(base, a, b), (cin, a, b)
            if kw:        # the products by k have no gate: exact for every a
                exact, ok = _int(a) * _int(kw), True
            elif "sqr" in cin:
                exact = sum(a[i] * a[j] << (32 * (i + j)) for i in range(8) for j in range(i + 1, 8))
                ok = max(a[0], a[7]) <= BOUND
            else:
                exact, ok = _int(a) * _int(b), max(a[0], b[7]) <= BOUND
            if ok:
                assert _int(got) == exact, (cin, a, b)
                n_exact += 1
            else:
                n_over += 1
    assert n_exact > 100 and (kw or n_over >= 4)


@pytest.mark.parametrize("base,cin", PAIRS)
def test_cin_form_is_the_in_place_form_but_for_the_carry_in_operand(base, cin):
    """Column by column the same instructions; a column reads %[cin] in its first product exactly when
    the column before it counted no carry (its carry-out's high word is zero), and then the C glue
    forms cin = acc >> 32 where the in-place form shifts acc."""
    sb, sc = _steps(base), _steps(cin)
    ab = [s for k, s in sb if k == "asm"]
    ac = [s for k, s in sc if k == "asm"]
    assert len(ab) == len(ac)
    split = 0
    for i, (x, y) in enumerate(zip(ab, ac)):
        prev_counted = i > 0 and any(t.startswith("v_addc_co_u32") for t in ab[i - 1])
        if i > 0 and not prev_counted:
            assert y[0] == x[0][:-len("%[acc]")] + "%[cin]" and x[0].endswith(", %[acc]") and y[1:] == x[1:]
            assert not any("%[cin]" in t for t in y[1:])
            split += 1
        else:
            assert x == y
    assert split == {"mul512_bounded_cin_asm": 1, "sqr512_offdiag_bounded_cin_asm": 3, "mul512_k_cin_asm": 5}[cin]
    cb = [s for k, s in sb if k == "c" and not s.startswith(("uint", "(void)"))]
    cc = [s for k, s in sc if k == "c" and not s.startswith(("uint", "(void)"))]
    shifts = [i for i, s in enumerate(cb) if s == "acc >>= 32"]   # (the last may follow the final column)
    assert len(shifts) - split in (0, 1)
    for i in shifts[:split]:
        cb[i] = "cin = acc >> 32"
    assert cc == cb
    # a split column's statement writes acc as an early-clobber output, so it cannot share cin's pair
    body = _body(cin)
    assert body.count('[cin] "v"(cin)') == split
    for m in re.finditer(r'asm volatile\("[^"]*%\[cin\][^;]*;', body):
        assert '[acc] "=&v"(acc)' in m.group(0)


def test_glue_gates_the_cin_forms_as_the_in_place_forms():
    src = open(os.path.join(CSRC, "fe25519_dev.h")).read()

    def after(fn, call):
        body = src[src.index(f"BP_DEV void {fn}("):]
        body = body[:body.index("\n}\n")]
        return [l.strip() for l in body[body.index(call) + len(call):].strip().splitlines()[:2]]
    assert after("mul512_cin", "mul512_bounded_cin_asm(w, a, b);") == after("mul512", "mul512_bounded_asm(w, a, b);")
    assert after("sqr512_cin", "sqr512_offdiag_bounded_cin_asm(o, a);") == after("sqr512", "sqr512_offdiag_bounded_asm(o, a);")
    for fn, old in (("fe_mul", "mul512"), ("fe_sq", "sqr512")):
        body = src[src.index(f"BP_DEV fe {fn}("):]
        body = body[:body.index("\n}\n")]
        assert f"if constexpr (LAT == 0 || LAT == 3) {old}_cin<LAT == 3 && BP_DEFER_GATES>(" in body
        assert f"    {old}<LAT == 3 && BP_DEFER_GATES>(" in body     # the latency forms and BP_MUL_CIN 0
    ge = open(os.path.join(CSRC, "ge25519_dev.h")).read()
    assert "if constexpr (BP_MUL_CIN && (LAT == 0 || LAT == 3)) mul512_k_cin_asm(w, a); else mul512_k_asm(w, a);" in ge
