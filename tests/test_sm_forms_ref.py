"""The CPU model of the drain-tick forms' chains (tests/sm_forms_ref.py) against the CPU restatement:
chain() itself asserts that its result is oracle.ge_scalarmult's, limb for limb; here it runs on the edge
base, a base that fails the product gate, a random base and the zero scalar, and the flags it reports are
the ones tests/test_sm_forms_gpu.py builds its cases on."""
import numpy as np

import sm_forms_ref as ref
from test_lane_defer_gpu import M32, _points, _with_top_word

EDGE_BASE = np.array([0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0], dtype=np.uint64)   # (X, Y, Z, T) = (0, 1, 1, 0)


def _scalar(rng, top=True):
    s = int.from_bytes(rng.bytes(32), "little")
    return s | (1 << 255) if top else s


def test_edge_base_flags_with_real_data(oracle):
    """(0, 1, 1, 0): X and T stay 0, so B - A = 0 and Y3 - X3 = Y3 is small in the first steps: the add/sub
    blocks' word-1 test fires at several in-loop steps, inside the step (what sm_row's ballot sees) too."""
    rng = np.random.default_rng(2100)
    got, steps = ref.chain(oracle, _scalar(rng), EDGE_BASE)
    assert len(steps) > 256 and steps[0]["op"] == "dbl" and steps[0]["bit"] == 255
    for blocks in (ref.EDGE_BLOCKS, ref.ROW_BLOCKS, ("addsub_BA",), ("addsub_DC",), ("addsub_next",)):
        assert len(ref.past_first_operation(steps, ref.edge_steps(steps, blocks))) >= 3, blocks


def test_random_base_flags_only_in_the_first_operation(oracle):
    rng = np.random.default_rng(2101)
    for affine in (True, False):
        s = _scalar(rng, top=False)
        _, steps = ref.chain(oracle, s, _points(rng, 1, affine)[0])
        assert len(steps) == s.bit_length() + bin(s).count("1")
        hits = ref.edge_steps(steps)
        assert 0 in hits                                    # the doubled identity's B - A = 0
        assert ref.past_first_operation(steps, hits) == []  # and nothing past the top bit's doubling and add
        assert ref.gate_steps(steps) == [] and ref.gate_steps(steps, q4=True) == []


def test_gate_base_fails_the_gate_at_every_add(oracle):
    """A base whose T has a top word above MUL_BOUNDED_WORD is the second factor of every add's T1 T2:
    fe_mul's gate (word 7 of the second factor) fails at each add and at no doubling; fe_mul_q4's gate reads
    the first factor only, so the row form's stays quiet."""
    rng = np.random.default_rng(2102)
    P = _with_top_word(rng, oracle, "T", 0xFFFFFFF0)
    _, steps = ref.chain(oracle, _scalar(rng), P)
    adds = [j for j, st in enumerate(steps) if st["op"] == "add"]
    assert len(adds) > 64 and ref.gate_steps(steps) == adds
    assert ref.gate_steps(steps, q4=True) == []
    P = _with_top_word(rng, oracle, "Y+X", M32)
    _, steps = ref.chain(oracle, _scalar(rng), P)
    assert ref.gate_steps(steps) == [j for j, st in enumerate(steps) if st["op"] == "add"]


def test_zero_and_short_scalars(oracle):
    """Scalar 0 has no in-loop step (the start state, the identity doubled 256 times, is the result);
    scalar 1 has the bit-0 doubling and its add; 5 flags nowhere past the first doubling."""
    rng = np.random.default_rng(2103)
    P = _points(rng, 1, False)[0]
    got, steps = ref.chain(oracle, 0, P)
    assert steps == []
    assert np.array_equal(got, np.asarray(oracle.ge_scalarmult(np.zeros(32, np.uint8), P), np.uint64))
    _, steps = ref.chain(oracle, 1, P)
    assert [(st["op"], st["bit"]) for st in steps] == [("dbl", 0), ("add", 0)]
    _, steps = ref.chain(oracle, 5, EDGE_BASE)
    assert [(st["op"], st["bit"]) for st in steps] == [("dbl", 2), ("add", 2), ("dbl", 1), ("dbl", 0), ("add", 0)]
