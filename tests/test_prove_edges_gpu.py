"""The provers and the verifiers on scalars outside the masked-random shape, bit for bit (np.array_equal on every
limb, no tolerance) against oracle.generate_range_proof, oracle.cuda_range_proof_verify and
oracle.range_proof_verify.  The inputs and the oracle's expectations come from tests/prove_edges.py (built once
per process); tests/test_prove_edges_cpu.py proves that each block reaches the path it is named for.

* the explicit prover on every block, plain and with prefix tables of 1, 8 and 12 bits: every output row of every
  proof, the documented zeroed rows where the value is refused;
* block A in reversed order: the same rows, reversed;
* the seeded, accepted and host provers on block C's value x blinding cross;
* every valid proof of blocks A, B and C through both batch verifiers;
* the verifiers on proofs whose t, taux, mu, x, c, a[0] or b[0] is an edge value.
"""
import numpy as np
import pytest

import prove_edges as pe
from test_gpu_parity import _run_batch, _run_std

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    dev = torch.device("cuda:0")
    return lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)


def _numpy(out, extra=()):
    return {k: (out[k].cpu().numpy() if k in ("valid", "attempts") else out[k].cpu().numpy().view(np.uint64))
            for k in pe.FIELDS + ("valid",) + tuple(extra)}


def _prove(bp, T, oracle, proofs, K=0):
    """batch_generate_range_proof on a list of input dicts (K > 0: through a Generators set with K-bit prefix
    tables) -> the outputs as numpy."""
    import torch
    n = proofs[0]["n"]
    ar = pe.arrays(proofs)
    G, H, g, h = (T(x) for x in pe.gens(oracle, n))
    gens = bp.Generators(n, G, H, g, h, prefix_bits=K) if K else None
    out = bp.batch_generate_range_proof(n, T(ar["v"]), T(ar["gamma"]), T(ar["sL"]), T(ar["sR"]), T(ar["rnd"]), G, H, g, h,
                                        gens=gens)
    torch.cuda.synchronize()
    got = _numpy(out)
    if gens is not None:
        gens.close()
    return got


@pytest.mark.parametrize("K", (0,) + pe.KS)
@pytest.mark.parametrize("key", list(pe.CALLS))
def test_explicit_prover_vs_oracle(bp, T, oracle, key, K):
    """valid, V, A, S, T1, T2, taux, mu, t, c, x, a, b, L and R of every proof of the call; a refused value's rows are
    the zeroed proof the header documents.  Failures are listed as (block, slot, e, field)."""
    proofs = pe.call(key)
    got = _prove(bp, T, oracle, proofs, K)
    bad = pe.mismatches(got, pe.oracle_proofs(oracle, key), [p["tag"] for p in proofs])
    assert not bad, (len(bad), bad[:12])


@pytest.mark.parametrize("n", [1, 2, 8, 64])
def test_refused_rows(bp, T, oracle, n):
    """Block C: where the oracle refuses the value, valid = 0 and every output row is what
    include/cudabulletproof_hip.h documents for hipbp_proof_out (V, A, S, T1, T2 the identity (0, 1, 1, 0); taux,
    mu, t, c, x, a, b and every limb of L and R zero), whatever the blinding; the valid neighbours in the same
    waves are the oracle's proofs."""
    proofs, want = pe.call(f"C{n}"), pe.oracle_proofs(oracle, f"C{n}")
    got = _prove(bp, T, oracle, proofs)
    refused = [p for p, w in enumerate(want) if w is None]
    assert len(refused) >= (25 if n >= 8 else 5) and len(refused) < len(want)
    zero = pe.refused_rows(n)
    for p in refused:
        assert got["valid"][p] == 0, proofs[p]["tag"]
        for k in pe.FIELDS:
            assert np.array_equal(got[k][p].reshape(zero[k].shape), zero[k]), (proofs[p]["tag"], k)
    keep = [p for p, w in enumerate(want) if w is not None]
    bad = pe.mismatches({k: v[keep] for k, v in got.items()}, [want[p] for p in keep], [proofs[p]["tag"] for p in keep])
    assert not bad, bad[:12]


@pytest.mark.parametrize("K", [0, 8])
def test_position_independence(bp, T, oracle, K):
    """Block A proven in reversed order gives the same rows, reversed: no proof's result depends on its place in
    the batch, its wave-mates' order or its rank in the work lists."""
    proofs = pe.call("A")
    fwd, rev = _prove(bp, T, oracle, proofs, K), _prove(bp, T, oracle, proofs[::-1], K)
    for k in pe.FIELDS + ("valid",):
        differ = np.nonzero((fwd[k] != rev[k][::-1]).reshape(len(proofs), -1).any(axis=1))[0]
        assert not len(differ), (k, [proofs[p]["tag"] for p in differ[:8]])


# ----------------------------------------------------------------------------- seeded, accepted and host forms
@pytest.mark.parametrize("n,cols", [(8, None), (64, ("0", "2^255"))])
def test_seeded_prover_vs_oracle(bp, T, oracle, n, cols):
    """batch_generate_range_proof_seeded on block C's (v, gamma) cross equals the oracle on the scalars
    tests/prove_seed_ref.py derives (the key binds v and gamma as stored, not canonicalised)."""
    import torch
    _, v, gamma, tags = pe.seeded_inputs(f"C{n}", cols)
    want = pe.seeded_proofs(oracle, f"C{n}", cols)
    assert len(v) == (60 if cols is None else 24) and any(w is None for w in want) and any(w is not None for w in want)
    G, H, g, h = (T(x) for x in pe.gens(oracle, n))
    out = bp.batch_generate_range_proof_seeded(n, T(v), T(gamma), pe.SEED, G, H, g, h, index_base=pe.IB)
    torch.cuda.synchronize()
    bad = pe.mismatches(_numpy(out), want, tags)
    assert not bad, bad[:12]


@pytest.mark.parametrize("check", [1, 2])
def test_accepted_prover_vs_cpu_loop(bp, T, oracle, check):
    """batch_generate_range_proof_accepted (n = 8, max_attempts = 4) on block C's cross: attempts and every row equal
    the CPU loop (tests/prove_try_ref.py's scalars, the oracle's prover and its verifier of `check`)."""
    n, v, gamma, tags = pe.seeded_inputs("C8")
    att, want = pe.accepted_proofs(oracle, "C8", check, 4)
    assert (att == 1).any() and (att >= 2).any() and any(w is None for w in want)   # accepts, a retry, refusals
    G, H, g, h = (T(x) for x in pe.gens(oracle, n))
    out = bp.batch_generate_range_proof_accepted(n, T(v), T(gamma), pe.SEED, G, H, g, h, index_base=pe.IB, max_attempts=4,
                                                 check=check)
    got = _numpy(out, extra=("attempts",))
    wrong = np.nonzero(got["attempts"] != att)[0]
    assert not len(wrong), [(tags[p], int(got["attempts"][p]), int(att[p])) for p in wrong[:8]]
    bad = pe.mismatches(got, want, tags)
    assert not bad, bad[:12]


def _structs_vs_oracle(proofs, valid, want, tags, n):
    Lr = n.bit_length() - 1
    zero_head = np.concatenate([pe.refused_rows(n)[k] for k in pe.HEAD])
    for p, (pr, w) in enumerate(zip(proofs, want)):
        assert bool(valid[p]) == (w is not None), tags[p]
        if w is None:   # the zeroed proof with an all-zero ip_proof
            assert np.array_equal(pr["head"], zero_head) and pr["n"] == 0 and pr["L_len"] == 0, tags[p]
            assert all(len(pr[k]) == 0 for k in ("a", "b", "L", "R")), tags[p]
            continue
        assert np.array_equal(pr["head"], w["head"]) and pr["n"] == n and pr["L_len"] == Lr, tags[p]
        for k in ("a", "b", "L", "R"):
            assert np.array_equal(pr[k], w[k].reshape(pr[k].shape)), (tags[p], k)


@pytest.mark.parametrize("shards", [None, 2])
def test_host_provers(bp, oracle, monkeypatch, shards):
    """batch_generate_range_proof_host and batch_generate_range_proof_accepted_host on block C's cross at n = 8, on one
    device and in two shards (HIPBP_HOST_SHARDS=2): the structs hold the oracle's proofs (the seeded scalars; the
    CPU loop's accepted attempt under check 1, max_attempts = 4), a refused value the zeroed one."""
    n, v, gamma, tags = pe.seeded_inputs("C8")
    if shards is None:
        monkeypatch.delenv("HIPBP_HOST_SHARDS", raising=False)
    else:
        monkeypatch.setenv("HIPBP_HOST_SHARDS", str(shards))
    ng = 1 if shards is None else 0
    gens = pe.gens(oracle, n)
    proofs, valid = bp.batch_generate_range_proof_host(v, gamma, n, *gens, pe.SEED, index_base=pe.IB, num_gpus=ng)
    _structs_vs_oracle(proofs, valid, pe.seeded_proofs(oracle, "C8"), tags, n)
    att, want = pe.accepted_proofs(oracle, "C8", 1, 4)
    proofs, valid, attempts = bp.batch_generate_range_proof_accepted_host(v, gamma, n, *gens, pe.SEED, index_base=pe.IB,
                                                                         max_attempts=4, check=1, num_gpus=ng)
    assert np.array_equal(attempts, att)
    _structs_vs_oracle(proofs, valid, want, tags, n)


# ----------------------------------------------------------------------------- prove, then verify
def _check_point_matters(ok, chk):
    """The oracle leaves the check point zero on an early reject (<a, b> != c), where the device writes none."""
    return ok or chk.any()


@pytest.mark.parametrize("key", ["A", "B", "C8"])
def test_prove_then_verify(bp, T, oracle, key):
    """Every valid proof of the call, as the GPU prover wrote it, through batch_range_proof_verify and
    batch_range_proof_verify_std: verdict, P and check point equal the oracle's verifiers on the oracle's proof.
    Here the verifiers meet taux, mu and t computed from non-canonical scalars."""
    proofs, want = pe.call(key), pe.verdicts(oracle, key)
    n = proofs[0]["n"]
    got = _prove(bp, T, oracle, proofs)
    keep = [p for p, w in enumerate(want) if w is not None]
    assert len(keep) >= 30 and all(got["valid"][p] == 1 for p in keep)
    ar = {k: np.ascontiguousarray(got[k][keep]) for k in pe.FIELDS}
    ar["Vp"] = ar["V"]
    gens = pe.gens(oracle, n)
    ok, Pt, chk = _run_batch(bp, n, ar, *gens)
    oks, Ps, chks = _run_std(bp, n, ar, *gens)[:3]
    bad = []
    for i, p in enumerate(keep):
        w, where = want[p], (proofs[p]["tag"][0], proofs[p]["tag"][1], pe.name(proofs[p]["tag"][2]))
        if ok[i] != w["ok"] or not np.array_equal(Pt[i], w["P"]) or \
                (_check_point_matters(w["ok"], w["check"]) and not np.array_equal(chk[i], w["check"])):
            bad.append(where + ("verify",))
        if oks[i] != w["ok_std"] or not np.array_equal(Ps[i], w["P_std"]) or \
                (_check_point_matters(w["ip_ok"], w["check_std"]) and not np.array_equal(chks[i], w["check_std"])):
            bad.append(where + ("verify_std",))
    assert not bad, (len(bad), bad[:12])


def test_verifier_scalar_edges(bp, oracle):
    """n = 4, 140 proofs with t, taux, mu, x, c, a[0] or b[0] replaced by a value of E among 47 untouched ones, through
    batch_range_proof_verify, batch_range_proof_verify_std and the single-proof cuda_range_proof_verify: verdict, P
    and check point against the oracle (the check point as test_batch_verify_synthetic_vs_oracle compares it)."""
    ar, heads, tags, want = pe.verifier_batch(oracle)
    gens = pe.gens(oracle, pe.VN)
    ok, Pt, chk = _run_batch(bp, pe.VN, ar, *gens)
    oks, Ps, chks, fl, _ = _run_std(bp, pe.VN, ar, *gens)
    bad = []
    for p, (w, tag) in enumerate(zip(want, tags)):
        where = (tag[0], tag[1], pe.name(tag[2]))
        if ok[p] != w["ok"] or not np.array_equal(Pt[p], w["P"]) or \
                (_check_point_matters(w["ok"], w["check"]) and not np.array_equal(chk[p], w["check"])):
            bad.append(where + ("verify",))
        det = w["det"]
        if oks[p] != w["ok_std"] or not np.array_equal(Ps[p], det["P"]) or bool(int(fl[p]) & 32) != det["ip_ok"] or \
                (_check_point_matters(det["ip_ok"], det["check"]) and not np.array_equal(chks[p], det["check"])):
            bad.append(where + ("verify_std",))
        proof = dict(head=heads[p], a=ar["a"][p], b=ar["b"][p], L=ar["L"][p], R=ar["R"][p])
        if bp.cuda_range_proof_verify(proof, ar["V"][p], pe.VN, *gens) != w["ok"]:
            bad.append(where + ("cuda_range_proof_verify",))
    assert not bad, (len(bad), bad[:12])
