"""GPU parity of the stand-alone IPA prover (hipbp_batch_inner_product_prove and its _gens / host
forms) against the reference's own inner_product_prove outputs in tests/golden/ipa_prove.npz
(tests/golden/make_ipa_prove.py; the inputs are derived here by the same recipe).  Everything is
bit-exact: this is integer arithmetic.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

NCASES = 25
NS = (1, 2, 4, 8, 64, 256, 4096)
OUT_KEYS = ("a", "b", "c", "x", "L", "R", "c_final")


class Env:
    """The fixture, the derived inputs of every case and the generators per n (host and device)."""

    def __init__(self, bp, golden, oracle):
        import torch
        from make_ipa_prove import CASES, case_inputs, generators
        assert len(CASES) == NCASES and tuple(sorted({n for n, _ in CASES})) == NS
        self.bp, self.torch, self.oracle = bp, torch, oracle
        self.dev = torch.device("cuda:0")
        self.d = golden("ipa_prove")
        self.cases = CASES
        self.inp = [case_inputs(k, n, r) for k, (n, r) in enumerate(CASES)]
        self.gen_np = {n: generators(oracle, n) for n in NS}
        self.gen = {n: tuple(self.T(x) for x in g) for n, g in self.gen_np.items()}

    def T(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(self.dev)

    def of_n(self, n):
        return [k for k, (m, _) in enumerate(self.cases) if m == n]

    def inputs(self, idx):
        a = np.stack([self.inp[k][0] for k in idx])
        b = np.stack([self.inp[k][1] for k in idx])
        tr = np.stack([self.inp[k][2].view("<u8") for k in idx])
        return self.T(a), self.T(b), self.T(self.d["c_in"][idx]), self.T(tr)

    def prove(self, idx, gens=None, stream=None, transcript=True):
        n = self.cases[idx[0]][0]
        a, b, c, tr = self.inputs(idx)
        G, H, Q = self.gen[n]
        return self.bp.batch_inner_product_prove(n, a, b, c, G, H, Q, transcript=tr if transcript else None,
                                                 stream=stream, gens=gens)

    def host(self, out):
        self.torch.cuda.synchronize()
        return {k: out[k].cpu().numpy().view(np.uint64) for k in OUT_KEYS}

    def want(self, idx):
        d, lo = self.d, self.d["L_off"]
        Lr = int(lo[idx[0] + 1] - lo[idx[0]])
        return dict(a=d["a"][idx][:, None], b=d["b"][idx][:, None], c=d["c_in"][idx], x=d["x"][idx],
                    c_final=d["c_final"][idx],
                    L=np.stack([d["L"][lo[k]:lo[k + 1]] for k in idx]).reshape(len(idx), Lr, 16),
                    R=np.stack([d["R"][lo[k]:lo[k + 1]] for k in idx]).reshape(len(idx), Lr, 16))

    def check(self, got, idx):
        want = self.want(idx)
        for k in OUT_KEYS:
            assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
            bad = [idx[p] for p in range(len(idx)) if not np.array_equal(got[k][p], want[k][p])]
            assert not bad, f"{k}: cases {bad[:8]} differ from the reference"


@pytest.fixture(scope="module")
def env(bp, golden, oracle):
    return Env(bp, golden, oracle)


def tile(idx, B):
    return [idx[p % len(idx)] for p in range(B)]


# ----------------------------------------------------------------------------- fixture parity
@pytest.mark.parametrize("case", range(NCASES))
def test_case_alone_matches_reference(env, case):
    """One proof per call: a, b, c, x, L, R, c_final bit for bit (n = 1: no rounds, x = 0)."""
    env.check(env.host(env.prove([case])), [case])


@pytest.mark.parametrize("n", NS)
def test_batch_of_equal_n_matches_reference(env, n):
    """All cases of one n in one call, in shuffled order.  n = 8: the random and the five edge cases
    (zero a; zero / light / heavy scalars in one proof; elements in [p, 2^255); a transcript with
    byte 31 >= 0x80; a c_in that is not <a, b>).  n = 256: B = 3, the first round's 4n' + 2 = 514
    items per proof straddle the 256-lane blocks.  n = 4096: both full-size instances in one call."""
    idx = env.of_n(n)
    idx = [idx[p] for p in np.random.default_rng(n).permutation(len(idx))]
    env.check(env.host(env.prove(idx)), idx)


def test_batch_67_n8(env):
    """B = 67 tiles the n = 8 cases: no multiple of a wave, and zero, light and heavy scalars of
    different proofs share waves."""
    idx = tile(env.of_n(8), 67)
    env.check(env.host(env.prove(idx)), idx)


def test_more_chunks_than_workspaces(env):
    """A 1 MB workspace budget cuts B = 24 at n = 256 into three chunks: the third reuses the first's
    workspace on the caller's stream behind it."""
    idx = tile(env.of_n(256), 24)
    old = os.environ.get("HIPBP_IPA_WS_MB")
    os.environ["HIPBP_IPA_WS_MB"] = "1"
    try:
        got = env.host(env.prove(idx))
    finally:
        if old is None:
            del os.environ["HIPBP_IPA_WS_MB"]
        else:
            os.environ["HIPBP_IPA_WS_MB"] = old
    env.check(got, idx)


def test_null_transcript_is_zeros(env):
    idx = [k for k in env.of_n(8) if env.cases[k][1] != 4]
    env.check(env.host(env.prove(idx, transcript=False)), idx)


# ----------------------------------------------------------------------------- generator sets
@pytest.mark.parametrize("n,bits,B", [(8, 6, 67), (256, 6, 3), (4096, 4, 2)])
def test_gens_form_has_the_plain_forms_bits(env, n, bits, B):
    idx = tile(env.of_n(n), B)
    G, H, Q = env.gen[n]
    g = env.T(env.oracle.gh()[0])
    gens = env.bp.Generators(n, G, H, g, Q, prefix_bits=bits)
    try:
        with_tables = env.host(env.prove(idx, gens=gens))
    finally:
        gens.close()
    plain = env.host(env.prove(idx))
    for k in OUT_KEYS:
        assert np.array_equal(with_tables[k], plain[k]), k
    env.check(with_tables, idx)


# ----------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("n", [64, 4096])
def test_round_trip_through_the_verifier(env, n):
    """prove -> P = msm_batch(a || b, G || H) -> batch_inner_product_verify with c_final and with c:
    the verdicts and the check point are the reference's (a proof rejected at c != <a, b> leaves no
    check point)."""
    torch, bp, d = env.torch, env.bp, env.d
    idx = env.of_n(n)[:2] if n == 4096 else env.of_n(n)
    B = len(idx)
    a, b, _, _ = env.inputs(idx)
    G, H, Q = env.gen[n]
    out = env.prove(idx)
    P = torch.zeros(B, 16, dtype=torch.int64, device=env.dev)
    bp.msm_batch(P, torch.cat([a, b], dim=1).contiguous(), torch.cat([G, H]).contiguous())
    torch.cuda.synchronize()
    assert np.array_equal(P.cpu().numpy().view(np.uint64), d["P"][idx])
    for which, want_ok in (("c_final", d["ok_final"][idx]), ("c", d["ok_in"][idx])):
        batch = bp.ipa_proof_batch(n, out, c=which)
        ok = torch.zeros(B, dtype=torch.uint8, device=env.dev)
        chk = torch.zeros(B, 16, dtype=torch.int64, device=env.dev)
        bp.batch_inner_product_verify(batch, P, G, H, Q, ok, chk)
        torch.cuda.synchronize()
        assert np.array_equal(ok.cpu().numpy().astype(bool), want_ok.astype(bool)), which
        if which == "c_final":
            assert np.array_equal(chk.cpu().numpy().view(np.uint64), d["check"][idx])


# ----------------------------------------------------------------------------- host form
def _host_call(env, a, b, G, H, Q, c, tr):
    bp = env.bp
    pr = bp.InnerProductProof()
    keep = [np.ascontiguousarray(x, np.uint64) for x in (a, b, G, H, Q, c)] + [np.ascontiguousarray(tr, np.uint8)]
    ptr = lambda x: x.ctypes.data
    av, bv = bp.FieldVector(ptr(keep[0]), len(keep[0])), bp.FieldVector(ptr(keep[1]), len(keep[1]))
    gv, hv = bp.PointVector(ptr(keep[2]), len(keep[2])), bp.PointVector(ptr(keep[3]), len(keep[3]))
    rc = bp.lib().hipbp_inner_product_prove_host(ctypes.byref(pr), ctypes.byref(av), ctypes.byref(bv),
                                                 ctypes.byref(gv), ctypes.byref(hv), ctypes.c_void_p(ptr(keep[4])),
                                                 ctypes.c_void_p(ptr(keep[5])), ctypes.c_void_p(ptr(keep[6])))
    return rc, pr


@pytest.mark.parametrize("case", [0, 9, 21])   # n = 1; n = 8 random; n = 8 with a non-zero transcript
def test_host_form_matches_reference(env, case):
    n = env.cases[case][0]
    a, b, tr, _ = env.inp[case]
    G, H, Q = env.gen_np[n]
    rc, pr = _host_call(env, a, b, G, H, Q, env.d["c_in"][case], tr)
    assert rc == 0
    Lr = n.bit_length() - 1
    assert (pr.n, pr.a.length, pr.b.length, pr.L.length, pr.R.length, pr.L_len) == (n, 1, 1, Lr, Lr, Lr)
    rd = lambda vec, w: np.ctypeslib.as_array(ctypes.cast(vec.elements, ctypes.POINTER(ctypes.c_uint64)),
                                              shape=(vec.length, w)).copy() if vec.length else np.zeros((0, w), np.uint64)
    got = dict(a=rd(pr.a, 4)[None], b=rd(pr.b, 4)[None], c=np.array(pr.c, np.uint64)[None],
               x=np.array(pr.x, np.uint64)[None], L=rd(pr.L, 16)[None], R=rd(pr.R, 16)[None])
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]
    for vec in (pr.a, pr.b, pr.L, pr.R):   # malloc'ed, as inner_product_proof_free expects
        libc.free(vec.elements)
    want = env.want([case])
    for k in got:
        assert np.array_equal(got[k], want[k]), k
    # and the numpy wrapper over the same entry point
    w = env.bp.inner_product_prove(a, b, G, H, Q, env.d["c_in"][case], tr)
    assert np.array_equal(w["a"], want["a"][0]) and np.array_equal(w["L"], want["L"][0]) and w["L_len"] == Lr
    assert np.array_equal(w["x"], want["x"][0]) and np.array_equal(w["c"], want["c"][0])


def test_host_form_length_mismatch_leaves_the_proof_untouched(env):
    a, b, tr, _ = env.inp[9]
    G, H, Q = env.gen_np[8]
    for args in ((a, b[:4], G, H), (a, b, G[:4], H), (a[:6], b[:6], G[:6], H[:6])):   # mismatches; n = 6
        rc, pr = _host_call(env, *args, Q, env.d["c_in"][9], tr)
        assert rc == 1
        assert bytes(pr) == bytes(ctypes.sizeof(pr))


# ----------------------------------------------------------------------------- arguments
def test_bad_arguments_write_nothing(env):
    bp, torch = env.bp, env.torch
    G, H, Q = env.gen[4]
    fill = lambda *s: torch.full(s, 0x5A5A5A5A, dtype=torch.int64, device=env.dev)
    a, b, c = fill(1, 4, 4), fill(1, 4, 4), fill(1, 4)
    outs = [fill(1, 4) for _ in range(5)] + [fill(1, 2, 16), fill(1, 2, 16)]
    oc = bp.IpaProofOutC(*[t.data_ptr() for t in outs])
    call = lambda ic: bp.lib().hipbp_batch_inner_product_prove(
        ctypes.byref(ic), ctypes.c_void_p(G.data_ptr()), ctypes.c_void_p(H.data_ptr()), ctypes.c_void_p(Q.data_ptr()),
        ctypes.byref(oc), None)
    assert call(bp.ProveIpaInputC(1, 3, a.data_ptr(), b.data_ptr(), c.data_ptr(), None)) == 1    # n = 3
    assert call(bp.ProveIpaInputC(1, 4, None, b.data_ptr(), c.data_ptr(), None)) == 1           # null a
    assert call(bp.ProveIpaInputC(1, 1 << 17, a.data_ptr(), b.data_ptr(), c.data_ptr(), None)) == 1
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 0x5A5A5A5A).all())
    with pytest.raises(bp.BulletproofError):
        bp.batch_inner_product_prove(3, a[:, :3], b[:, :3], c, G, H, Q)


# ----------------------------------------------------------------------------- streams
def test_two_streams_at_once(env):
    """The n = 64 batch on two streams at once, twice: each stream has its own workspace pair and
    side stream.  Then the workspaces of one stream are released and the call repeated."""
    torch = env.torch
    idx = env.of_n(64)
    rev = idx[::-1]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        with torch.cuda.stream(s1):
            o1 = env.prove(idx, stream=s1)
        with torch.cuda.stream(s2):
            o2 = env.prove(rev, stream=s2)
        outs.append((o1, o2))
    for o1, o2 in outs:
        env.check(env.host(o1), idx)
        env.check(env.host(o2), rev)
    env.bp.release_stream_workspaces(s1)
    with torch.cuda.stream(s1):
        o1 = env.prove(idx, stream=s1)
    env.check(env.host(o1), idx)
    env.bp.release_stream_workspaces(s1)
    env.bp.release_stream_workspaces(s2)
