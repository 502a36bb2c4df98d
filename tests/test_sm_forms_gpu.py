"""The drain-tick scalar-multiplication forms (ge25519_quad.h sm_quad, sm_pair, sm_row) on the device through
bp.sm_form_probe, bit for bit (all 16 limbs, np.array_equal, no tolerance) against oracle.ge_scalarmult, on
inputs the pipeline tests never feed them:

* random items, and the same items through the per-lane form (bp.sm_probe);
* counts that leave idle items in a wave and cross the wave and the block boundary, `out` guarded by a sentinel;
* scalar shapes mixed inside one wave: 0 (the i < 0 early return beside running wave-mates), 1, 2^255,
  2^256 - 1, alternating bits, lengths around every 64-bit word boundary (the bit stream's refill, which the
  rows of a wave then cross at different steps), long doubling and add runs; equal scalars as neighbours and
  interleaved;
* the edge base (0, 1, 1, 0) at each item position of a 16-lane DPP row: its add/sub blocks sit on
  fe25519_sub's rare edge for several steps, which for the row form is the deferred recompute on real data
  (beside three bystander rows), for quads and pairs the gated blocks' exact forms;
* bases that fail the product gate at every add (quads and pairs: fe_mul's gate reads the second factor's
  top word; the row form's fe_mul_q4 reads its first factor only, so there the same bases are the extreme
  second factor of the quad-split product);
* rows with every step of every chain forced through the recompute (force = 1): the same bits;
* the argument errors, refused before any launch;
* one small batch through the verify pipeline under each tick form and through the drop-in, with an edge base
  and gate-failing bases among the generators.

tests/sm_forms_ref.py (a CPU model of one chain) proves for each constructed case that it reaches the path
it is named for; a case that stops reaching it fails here.
"""
import numpy as np
import pytest

import sm_forms_ref as ref
from test_lane_defer_gpu import M32, _T, _points, _probe, _sm_oracle, _with_top_word
from test_lane_vote_gpu import _limbs, _wave

pytestmark = pytest.mark.gpu

FORMS = (1, 2, 3)               # HIPBP_QUAD's values: quads, pairs, rows
LANES = {1: 4, 2: 2, 3: 16}     # lanes per item
TPB = 256                       # bp_kernels.hip: the probe's block
SENTINEL = 0x5EA1ED5EA1ED5EA1
EDGE_BASE = np.array([0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0], dtype=np.uint64)   # (X, Y, Z, T) = (0, 1, 1, 0)
GATE_SPECS = [("T", 0xFFFFFFF0), ("Y+X", M32), ("Z", M32), ("Y+X", 0xFFFFFFF0)]   # test_lane_vote_gpu's `gate` case

_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _form_probe(bp, form, force, s, P, guard=0):
    """out (len(s) + guard, 16) after the probe of len(s) items; the guard rows must keep the sentinel."""
    import torch
    out = torch.full((len(s) + guard, 16), SENTINEL, dtype=torch.int64, device="cuda:0")
    bp.sm_form_probe(form, force, out, _T(s), _T(P))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


def _bad(got, want):
    return np.nonzero((got != want).any(axis=1))[0]


def _scalars(ints):
    return np.array([_limbs(x) for x in ints], dtype=np.uint64)


# ----------------------------------------------------------------------------- the blocks (built once)
def _random_block(oracle):
    def make():
        rng = np.random.default_rng(2200)
        s = rng.integers(0, 2**64, size=(256, 4), dtype=np.uint64)
        P = np.concatenate([_points(rng, 128, True), _points(rng, 128, False)])
        return s, P, _sm_oracle(oracle, s, P)
    return _memo("random", make)


def _shape_list(rng):
    R = lambda: int.from_bytes(rng.bytes(32), "little")
    shapes = [0, 1, 1 << 255, (1 << 256) - 1, int("AA" * 32, 16), int("55" * 32, 16)]
    for bits in (1, 63, 64, 65, 128, 129, 192, 193):      # exactly `bits` long: the refill crosses each word boundary
        shapes.append((1 << (bits - 1)) | (R() & ((1 << (bits - 1)) - 1)))
    shapes += sorted(set(_wave("runs", rng)))              # sparse / dense, differing in a few low bits
    assert len(shapes) == 18 and [x.bit_length() for x in shapes[6:14]] == [1, 63, 64, 65, 128, 129, 192, 193]
    return shapes


def _shapes_block(oracle):
    """72 items: the 18 shapes twice with equal scalars as neighbours, then twice interleaved (so the four rows,
    16 quads or 32 pairs of a wave disagree); each layout's first copy-half on Z = 1 bases, the rest on Z != 1."""
    def make():
        rng = np.random.default_rng(2201)
        shapes = _shape_list(rng)
        order = [x for x in shapes for _ in range(2)] + [shapes[i % 18] for i in range(36)]
        s = _scalars(order)
        P = np.concatenate([_points(rng, 18, True), _points(rng, 18, False), _points(rng, 18, True),
                            _points(rng, 18, False)])
        for k in range(0, 36, 2):
            assert np.array_equal(s[k], s[k + 1])
        for k in range(36, 71):
            assert not np.array_equal(s[k], s[k + 1])
        return s, P, _sm_oracle(oracle, s, P)
    return _memo("shapes", make)


def _pool(oracle):
    """32 random bystander items (half on Z = 1 bases, alternating) and the model's verdict on each: no
    rare-edge flag past the chain's first operation, no failed gate anywhere."""
    def make():
        rng = np.random.default_rng(2202)
        s = rng.integers(0, 2**64, size=(32, 4), dtype=np.uint64)
        P = _points(rng, 32, False)
        P[::2, 8:12] = 0
        P[::2, 8] = 1
        clean = []
        for k in range(32):
            _, steps = ref.chain(oracle, s[k], P[k])
            clean.append(len(ref.past_first_operation(steps, ref.edge_steps(steps))))
            assert ref.gate_steps(steps) == [] and ref.gate_steps(steps, q4=True) == [], k
        return s, P, clean
    return _memo("pool", make)


def _slot(form, wave):
    """The item of wave `wave` that carries the constructed base.  Rows: row `wave` of the wave's four.  Quads
    and pairs: position `wave` among the 4 quads / 8 pairs of a 16-lane DPP row, in another DPP row each time."""
    if form == 3:
        return wave
    per_row = 16 // LANES[form]
    assert wave < per_row
    return per_row * ((wave + 1) % 4) + wave


def _edge_block(oracle, form):
    """One wave per item position of a DPP row (4 rows / 4 quads / 8 pairs): bystanders from the pool, rotated,
    and at that position the edge base under a scalar with bit 255 set."""
    def make():
        rng = np.random.default_rng(2203 + form)
        ps, pP, clean = _pool(oracle)
        ipw = 64 // LANES[form]
        waves = 4 if form != 2 else 8
        s, P, slots, counts = [], [], [], []
        for w in range(waves):
            idx = [(k + 5 * w) % 32 for k in range(ipw)]
            ws, wP = ps[idx].copy(), pP[idx].copy()
            assert not any(clean[k] for k in idx)            # bystanders: nothing past the first operation
            at = _slot(form, w)
            assert at < ipw
            ws[at] = rng.integers(0, 2**64, size=4, dtype=np.uint64)
            ws[at, 3] |= np.uint64(1 << 63)
            wP[at] = EDGE_BASE
            _, steps = ref.chain(oracle, ws[at], wP[at])
            blocks = ref.ROW_BLOCKS if form == 3 else ref.EDGE_BLOCKS
            hits = ref.past_first_operation(steps, ref.edge_steps(steps, blocks))
            assert len(hits) >= 3, (form, w, hits)          # the recompute / the exact forms, on real data
            counts.append(len(hits))
            slots.append(ipw * w + at)
            s.append(ws)
            P.append(wP)
        s, P = np.concatenate(s), np.concatenate(P)
        print(f"edge block, form {form}: flagged in-loop steps past the first operation: edge items {counts}, "
              f"bystanders {sorted(set(clean))}")
        return s, P, _sm_oracle(oracle, s, P), slots
    return _memo(("edge", form), make)


# ----------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("form", FORMS)
def test_random_items(bp, oracle, form):
    """256 random scalars, half on Z = 1 bases: the oracle's bits, and the per-lane form's."""
    s, P, want = _random_block(oracle)
    got = _form_probe(bp, form, 0, s, P)
    assert np.array_equal(got, want), _bad(got, want)
    assert np.array_equal(got, _probe(bp, 0, s, P))


@pytest.mark.parametrize("case", ["lone", "idle", "wave", "block"])
@pytest.mark.parametrize("form", FORMS)
def test_counts_and_tails(bp, oracle, form, case):
    """A lone item, a wave with idle items, counts just past the wave and the block boundary: every stored
    item is the oracle's and the rows of `out` past count keep the sentinel."""
    L = LANES[form]
    count = {"lone": 1, "idle": 5, "wave": 64 // L + 3, "block": TPB // L + 1}[case]
    s, P, want = _random_block(oracle)
    pick = np.arange(count) * 131 % 256   # distinct items, both kinds of base
    got = _form_probe(bp, form, 0, s[pick], P[pick], guard=3)
    assert np.array_equal(got[:count], want[pick]), _bad(got[:count], want[pick])
    assert (got[count:] == np.uint64(SENTINEL)).all()


@pytest.mark.parametrize("form", FORMS)
def test_scalar_shapes_mixed_in_a_wave(bp, oracle, form):
    s, P, want = _shapes_block(oracle)
    got = _form_probe(bp, form, 0, s, P)
    assert np.array_equal(got, want), _bad(got, want)


@pytest.mark.parametrize("form", FORMS)
def test_edge_base_at_each_position_of_a_dpp_row(bp, oracle, form):
    """Every chain meets the rare-edge test once, in its first operation (the doubled identity); the edge
    item meets it at several later steps too (the model: at least 3, _edge_block), while its wave-mates are
    in mid-chain on ordinary points.  For rows the whole wave then reruns the step (ge_row_of_step<BP_ROW_LAT>)
    and takes its DPP broadcasts from the rerun.  The blocks' test is a superset of the inputs on which their
    fast statements differ from the exact ones, so this pins the path taken, not a wrong fast result."""
    s, P, want, slots = _edge_block(oracle, form)
    got = _form_probe(bp, form, 0, s, P)
    assert np.array_equal(got[slots], want[slots]), (slots, _bad(got[slots], want[slots]))
    assert np.array_equal(got, want), _bad(got, want)        # and every bystander


@pytest.mark.parametrize("form", FORMS)
def test_gate_failing_bases(bp, oracle, form):
    """One item per wave on a base whose T, Z or Y + X has a top word above MUL_BOUNDED_WORD.  In the quad and
    pair steps that operand is the second factor of a stage-1 product of every add, whose gate fails there
    and nowhere else (the model).  The row step's products are fe_mul_q4, whose gate reads the words of its
    first factor, the running point's operand: the base cannot fail it (the model shows that too), and what
    runs is the quad-split partial products against a second factor with an extreme top word."""
    rng = np.random.default_rng(2210 + form)
    ps, pP, _ = _pool(oracle)
    ipw = 64 // LANES[form]
    s, plain, slots = [], [], []
    for w in range(4):   # waves 0, 1: every base has Z = 1 (the pool's even items); waves 2, 3: Z != 1 around the slot
        idx = [(2 * (k + 3 * w) + (w >= 2)) % 32 for k in range(ipw)]
        s.append(ps[idx])
        plain.append(pP[idx])
        slots.append(ipw * w + (w * 23 + 9) % ipw)
    s, plain = np.concatenate(s), np.concatenate(plain)
    quirk = plain.copy()
    for at, (coord, word) in zip(slots, GATE_SPECS):
        quirk[at] = _with_top_word(rng, oracle, coord, word)
        _, steps = ref.chain(oracle, s[at], quirk[at])
        adds = [j for j, st in enumerate(steps) if st["op"] == "add"]
        assert len(adds) > 64 and ref.gate_steps(steps) == adds, (coord, hex(word))
        assert ref.gate_steps(steps, q4=True) == []
    want = _sm_oracle(oracle, s, quirk)
    got = _form_probe(bp, form, 0, s, quirk)
    assert np.array_equal(got, want), _bad(got, want)
    other = [i for i in range(len(s)) if i not in slots]
    assert np.array_equal(got[other], _form_probe(bp, form, 0, s, plain)[other])


@pytest.mark.parametrize("block", ["random", "shapes", "edge"])
def test_rows_forced_through_the_recompute(bp, oracle, block):
    """force = 1: every step of every chain is ge_row_of_step<BP_ROW_LAT> after the deferred pass, the steps
    right after a refill and the last one before an exit among them.  All items are compared, with the
    unforced run and with the oracle."""
    s, P, want = {"random": _random_block, "shapes": _shapes_block, "edge": lambda o: _edge_block(o, 3)}[block](oracle)[:3]
    forced, normal = _form_probe(bp, 3, 1, s, P), _form_probe(bp, 3, 0, s, P)
    assert forced.shape == want.shape                        # every item of the block
    assert np.array_equal(forced, normal), _bad(forced, normal)
    assert np.array_equal(forced, want), _bad(forced, want)


@pytest.mark.parametrize("form,force", [(0, 0), (4, 0), (1, 1), (2, 1), (3, 2)])
def test_argument_errors(bp, oracle, form, force):
    s, P, _ = _random_block(oracle)
    import torch
    out = torch.full((8, 16), SENTINEL, dtype=torch.int64, device="cuda:0")
    with pytest.raises(bp.BulletproofError, match="sm_form_probe: (form|force)"):
        bp.sm_form_probe(form, force, out, _T(s[:8]), _T(P[:8]))
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint64) == np.uint64(SENTINEL)).all()


def test_pipeline_and_drop_in_on_edge_generators(bp, oracle, monkeypatch):
    """n = 4, B = 3 synthetic proofs whose generators hold the edge base (G[1]) and two gate-failing bases
    (H[2], g), proof 0 under an x with bit 255 set: stage0_job / fold_job feeding each tick form, and the
    normalisation after it.  Verdict, P and check point of every proof under HIPBP_QUAD = 0, 1, 2, 3 and the
    drop-in's verdicts (the row form) against oracle.cuda_range_proof_verify."""
    from cudabulletproof_amd import synth
    from test_gpu_parity import _pipeline_outputs
    n, B = 4, 3
    rng = np.random.default_rng(2220)
    G, H = oracle.base_points(n, 1).copy(), oracle.base_points(n, 2).copy()
    g, h = (np.array(v, np.uint64) for v in oracle.gh())
    G[1] = EDGE_BASE
    H[2] = _with_top_word(rng, oracle, "T", 0xFFFFFFF0)
    g = _with_top_word(rng, oracle, "Z", M32)
    arrays = synth.proofs(B, n, seed=2221)
    arrays["x"][0, 3] |= np.uint64(1 << 63)
    heads = [np.concatenate([arrays[k][p] for k in ("V", "A", "S", "T1", "T2")] +
                            [np.zeros(8, np.uint64), arrays["t"][p], arrays["c"][p], arrays["x"][p]]) for p in range(B)]
    want = [oracle.cuda_range_proof_verify(heads[p], arrays["V"][p], n, arrays["a"][p], arrays["b"][p], arrays["L"][p],
                                           arrays["R"][p], G, H, g, h)[:3] for p in range(B)]
    for q in ("0", "1", "2", "3"):
        monkeypatch.setenv("HIPBP_QUAD", q)
        ok, P, chk = _pipeline_outputs(bp, n, B, 1, arrays, G, H, g, h, None)[-1][:3]
        ok, P, chk = ok.numpy().astype(bool), P.numpy().view(np.uint64), chk.numpy().view(np.uint64)
        for p in range(B):
            assert ok[p] == want[p][0] and np.array_equal(P[p], want[p][1]) and np.array_equal(chk[p], want[p][2]), (q, p)
    monkeypatch.delenv("HIPBP_QUAD")
    for p in range(B):
        proof = dict(head=heads[p], a=arrays["a"][p], b=arrays["b"][p], L=arrays["L"][p], R=arrays["R"][p])
        assert bp.cuda_range_proof_verify(proof, arrays["V"][p], n, G, H, g, h) == bool(want[p][0]), p
