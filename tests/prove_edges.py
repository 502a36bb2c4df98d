"""Prover and verifier inputs outside the masked-random scalar shape: the input builder, a CPU model of
the prover's data-dependent paths, and the oracle's expectations (computed once per process and shared
by tests/test_prove_edges_cpu.py and tests/test_prove_edges_gpu.py).  Not a test module.

Every prover test before these drew gamma, sL, sR, alpha, rho, tau1, tau2 in generate_random_scalar's
shape (bit 255 clear, bit 254 set, the low three bits clear), but hipbp_batch_generate_range_proof takes
any 32 bytes.  The blocks below put the edge list E and scalars around each prefix-table width's boundary
into every slot, alone and in whole vectors, cross edge values with edge blindings, make a wave's scalars
uniform, and empty the work lists.

The model restates, on Python integers, what bp_prove.hip and ge25519_dev.h decide from a scalar:
sclass (constant / light / heavy), fe_clz256, sm_ops_prefix's key and prefix_index.  sL, sR, v and gamma
are classified in canonical form (oracle.fe_tobytes, the device's fe_canon), alpha and rho as the raw
bytes, as terms0_scalar hands them out.
"""
import numpy as np

from oracle.pyoracle import head_fields, prover_randomness

import prove_seed_ref as sref
import prove_try_ref as tref

P = 2**255 - 19
E = [0, 1, 2, 8, 2**63, 2**64 - 1, 2**64, 2**64 + 1, 2**128, 2**192 - 1, P - 1, P, P + 1, P + 2**64, 2**255 - 1, 2**255,
     2**255 + 1, 2 * P, 2 * P + 1, 2**256 - 1]
KS = (1, 8, 12)                      # the prefix-table widths the GPU tests run
SLOTS = ("gamma", "alpha", "rho", "tau1", "tau2", "sL[0]", "sL[n-1]", "sR[0]", "sR[n-1]")
RND = ("alpha", "rho", "tau1", "tau2")
KINDS = ("sL", "sR", "gamma", "alpha", "rho")     # the slot kinds k_prove_prep classifies (v apart)
RAW_KINDS = ("alpha", "rho")
FIELDS = ("V", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x", "a", "b", "L", "R")
HEAD = ("V", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x")
SEED = bytes(range(32))              # the seeded provers' seed
IB = 7                               # and their index_base
V0 = 0xA5


def _boundary():
    """For each K: values of exact bit length 255 - K, 256 - K, 257 - K (clz = K + 1, K, K - 1), seeded lower bits."""
    rng = np.random.default_rng(2300)
    out = []
    for K in KS:
        for bits in (255 - K, 256 - K, 257 - K):
            low = int.from_bytes(rng.bytes(32), "little") & ((1 << (bits - 1)) - 1)
            out.append((1 << (bits - 1)) | low)
            assert out[-1].bit_length() == bits
    return out


BOUNDARY = _boundary()
assert len(E) == 20 and len(set(E)) == 20 and len(BOUNDARY) == 9


# ----------------------------------------------------------------------------- integers <-> arrays
def limbs(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), "<u8").astype(np.uint64)


def b32(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), np.uint8)


def _int(b):
    return int.from_bytes(bytes(np.ascontiguousarray(b)), "little")


def name(e):
    """A readable name of a scalar for failure reports."""
    if e is None:
        return "-"
    if e in E_NAMES:
        return E_NAMES[e]
    for base, tag in ((2**256, "2^256"), (2 * P, "2p"), (2**255, "2^255"), (P, "p"), (2**192, "2^192"), (2**128, "2^128"),
                      (2**64, "2^64"), (2**63, "2^63"), (0, "")):
        d = e - base
        if abs(d) <= 2**16:
            return (tag + (f"{d:+d}" if d else "")) if tag else str(e)
    return f"0x{e:x}"


E_NAMES = dict(zip(E, "0 1 2 8 2^63 2^64-1 2^64 2^64+1 2^128 2^192-1 p-1 p p+1 p+2^64 2^255-1 2^255 2^255+1 2p 2p+1 "
                      "2^256-1".split()))


# ----------------------------------------------------------------------------- proofs' inputs
def ordinary(n, v, seed, tag):
    """One proof's inputs with every scalar from prover_randomness(seed, n): dict(n, v, gamma, sL, sR, rnd, tag),
    the scalars Python integers of up to 256 bits; tag = (block, slot, e)."""
    gamma, sLR, rnd4 = prover_randomness(seed, n)
    return dict(n=n, v=v, gamma=_int(gamma), sL=[_int(sLR[i, :32]) for i in range(n)],
                sR=[_int(sLR[i, 32:]) for i in range(n)], rnd=[_int(rnd4[k]) for k in range(4)], tag=tag)


def set_slot(pr, slot, e):
    n = pr["n"]
    if slot == "gamma":
        pr["gamma"] = e
    elif slot in RND:
        pr["rnd"][RND.index(slot)] = e
    else:
        pr[slot[:2]][0 if slot.endswith("[0]") else n - 1] = e


def block_A(n=8):
    """One slot at a time: each slot x each value of E and of the boundary list, an ordinary proof after every
    third one (so edge lanes share waves with ordinary ones)."""
    out, k = [], 0
    for slot in SLOTS:
        for e in E + BOUNDARY:
            pr = ordinary(n, V0, 7000 + len(out), ("A", slot, e))
            set_slot(pr, slot, e)
            out.append(pr)
            k += 1
            if k % 3 == 0:
                out.append(ordinary(n, V0, 7000 + len(out), ("A", "ordinary", None)))
    return out


def block_B(n=8):
    """Whole vectors: for each e all sL = e; all sR = e; every scalar of the proof = e."""
    out = []
    for e in E:
        for what in ("sL[*]", "sR[*]", "all"):
            pr = ordinary(n, V0, 7600 + len(out), ("B", what, e))
            if what in ("sL[*]", "all"):
                pr["sL"] = [e] * n
            if what in ("sR[*]", "all"):
                pr["sR"] = [e] * n
            if what == "all":
                pr["gamma"], pr["rnd"] = e, [e] * 4
            out.append(pr)
    return out


def c_values(n):
    if n <= 2:
        return [0, 1, 2, P, 2**256 - 1]
    return [0, 1, 2**n - 1, 2**(n - 1), 2**n, P, P + 1, P + 2**n - 1, 2**255, 2**255 + 5, 2 * P + 3, 2**256 - 1]


def c_gammas(n):
    """(name, gamma): 0, 1, p, 2^255 and one masked-random blinding."""
    return [("0", 0), ("1", 1), ("p", P), ("2^255", 2**255), ("masked", _int(prover_randomness(7900, n)[0]))]


def block_C(n):
    """Values x blindings, gamma-major; the other scalars ordinary."""
    out = []
    for gname, gamma in c_gammas(n):
        for v in c_values(n):
            pr = ordinary(n, v, 8000 + 100 * n + len(out), ("C", f"n={n} gamma={gname} v", v))
            pr["gamma"] = gamma
            out.append(pr)
    return out


D_HEAVY = _int(prover_randomness(8900, 8)[0])      # a heavy scalar that is no edge


def block_D(common, n=8, B=70):
    """One wave plus six proofs: sL, sR, gamma, alpha, rho all = common, tau1 and tau2 fixed, only v differs."""
    fixed = ordinary(n, 0, 8901, None)
    out = []
    for p in range(B):
        out.append(dict(n=n, v=p, gamma=common, sL=[common] * n, sR=[common] * n,
                        rnd=[common, common, fixed["rnd"][2], fixed["rnd"][3]], tag=("D", f"common={name(common)} v", p)))
    return out


def block_E(which, n=8):
    """(a) every scalar 0 and v = 0, B = 3; (b) every scalar light (non-zero, <= 64 bits), B = 5; (c) B = 1
    ordinary; (d) B = 65 ordinary, proof 64 alone all zero."""
    zero = lambda p: dict(n=n, v=0, gamma=0, sL=[0] * n, sR=[0] * n, rnd=[0] * 4, tag=("E", which + " zero", p))
    if which == "a":
        return [zero(p) for p in range(3)]
    if which == "b":
        rng = np.random.default_rng(2301)
        lt = lambda: int(rng.integers(1, 2**63)) * 2 + 1
        return [dict(n=n, v=V0 + p, gamma=lt(), sL=[lt() for _ in range(n)], sR=[lt() for _ in range(n)],
                     rnd=[lt() for _ in range(4)], tag=("E", "b light", p)) for p in range(5)]
    if which == "c":
        return [ordinary(n, V0, 9300, ("E", "c ordinary", 0))]
    assert which == "d"
    return [ordinary(n, V0, 9400 + p, ("E", "d ordinary", p)) for p in range(64)] + [zero(64)]


CALLS = {"A": block_A, "B": block_B, "C1": lambda: block_C(1), "C2": lambda: block_C(2), "C8": lambda: block_C(8),
         "C64": lambda: block_C(64), "D": lambda: block_D(D_HEAVY), "D255": lambda: block_D(2**255 + 1),
         "Ea": lambda: block_E("a"), "Eb": lambda: block_E("b"), "Ec": lambda: block_E("c"), "Ed": lambda: block_E("d")}

_cache = {}


def memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def call(key):
    """The proofs of one prover call (a list of input dicts, all of one n)."""
    return memo(("call", key), CALLS[key])


def arrays(proofs):
    """hipbp_prove_input's arrays: v, gamma (B,4), sL, sR (B,n,4), rnd (B,4,4) uint64."""
    n = proofs[0]["n"]
    return dict(v=np.stack([limbs(p["v"]) for p in proofs]), gamma=np.stack([limbs(p["gamma"]) for p in proofs]),
                sL=np.stack([np.stack([limbs(x) for x in p["sL"]]) for p in proofs]).reshape(-1, n, 4),
                sR=np.stack([np.stack([limbs(x) for x in p["sR"]]) for p in proofs]).reshape(-1, n, 4),
                rnd=np.stack([np.stack([limbs(x) for x in p["rnd"]]) for p in proofs]))


def gens(oracle, n):
    def make():
        g, h = oracle.gh()
        return oracle.base_points(n, 1), oracle.base_points(n, 2), np.array(g, np.uint64), np.array(h, np.uint64)
    return memo(("gens", n), make)


# ----------------------------------------------------------------------------- the oracle's expectations
def oracle_proof(oracle, pr):
    n = pr["n"]
    sLR = np.stack([np.concatenate([b32(pr["sL"][i]), b32(pr["sR"][i])]) for i in range(n)])
    return oracle.generate_range_proof(b32(pr["v"]), b32(pr["gamma"]), sLR, np.stack([b32(x) for x in pr["rnd"]]), n,
                                       *gens(oracle, n))


def oracle_proofs(oracle, key):
    """oracle.generate_range_proof of every proof of call `key`: a list of dicts, None where refused."""
    return memo(("proofs", key), lambda: [oracle_proof(oracle, pr) for pr in call(key)])


def refused_rows(n):
    """What include/cudabulletproof_hip.h documents for valid = 0 (hipbp_proof_out): V, A, S, T1, T2 the
    identity (0, 1, 1, 0); taux, mu, t 0; the rest (c, x, a, b, every L and R limb) 0."""
    Lr = max(n.bit_length() - 1, 0)
    ident = np.zeros(16, np.uint64)
    ident[4] = ident[8] = 1
    d = {k: ident for k in HEAD[:5]}
    d.update({k: np.zeros(4, np.uint64) for k in HEAD[5:]})
    d.update(a=np.zeros((1, 4), np.uint64), b=np.zeros((1, 4), np.uint64), L=np.zeros((Lr, 16), np.uint64),
             R=np.zeros((Lr, 16), np.uint64))
    return d


def rows(pr, n):
    """An oracle proof (or None: refused) as the prover's output rows, by field."""
    if pr is None:
        return refused_rows(n)
    d = dict(head_fields(pr["head"]))
    d.update(a=pr["a"].reshape(1, 4), b=pr["b"].reshape(1, 4), L=pr["L"].reshape(-1, 16), R=pr["R"].reshape(-1, 16))
    return d


def mismatches(got, want, tags):
    """got: the prover's outputs as numpy (field -> (B, ...) uint64, valid (B,)); want: the oracle's proofs.
    Returns the failures as (block, slot, e, field)."""
    bad = []
    for p, (w, tag) in enumerate(zip(want, tags)):
        n = got["L"].shape[1]
        where = (tag[0], tag[1], name(tag[2]))
        if int(got["valid"][p]) != int(w is not None):
            bad.append(where + ("valid",))
        r = rows(w, 1 << n)
        for k in FIELDS:
            if not np.array_equal(np.asarray(got[k][p]).reshape(r[k].shape), r[k]):
                bad.append(where + (k,))
    return bad


def verdicts(oracle, key):
    """Both oracle verifiers on every valid proof of call `key` -> list of None (refused) or
    dict(ok, P, check, ok_std, P_std, check_std, ip_ok)."""
    def make():
        out = []
        for pr, w in zip(call(key), oracle_proofs(oracle, key)):
            if w is None:
                out.append(None)
                continue
            n = pr["n"]
            args = (w["head"], w["V"], n, w["a"], w["b"], w["L"], w["R"]) + gens(oracle, n)
            ok, Pt, chk = oracle.cuda_range_proof_verify(*args)[:3]
            oks, det = oracle.range_proof_verify(*args)
            out.append(dict(ok=ok, P=Pt, check=chk, ok_std=oks, P_std=det["P"], check_std=det["check"], ip_ok=det["ip_ok"]))
        return out
    return memo(("verdicts", key), make)


def seeded_inputs(key, cols=None):
    """Block C's (v, gamma) cross as the seeded provers' inputs: (n, v (B,4), gamma (B,4), tags); cols: keep only
    the blindings with these names."""
    prs = [p for p in call(key) if cols is None or any(f"gamma={c} " in p["tag"][1] for c in cols)]
    return prs[0]["n"], np.stack([limbs(p["v"]) for p in prs]), np.stack([limbs(p["gamma"]) for p in prs]), \
        [p["tag"] for p in prs]


def _prove_with(oracle, n, v, gamma, sc):
    sLR = np.concatenate([sc["sL"].view(np.uint8).reshape(n, 32), sc["sR"].view(np.uint8).reshape(n, 32)], axis=1)
    return oracle.generate_range_proof(np.ascontiguousarray(v).view(np.uint8), np.ascontiguousarray(gamma).view(np.uint8),
                                       sLR, sc["rnd"].view(np.uint8).reshape(4, 32), n, *gens(oracle, n))


def seeded_proofs(oracle, key, cols=None):
    """The oracle's proofs on the scalars tests/prove_seed_ref.py derives for seeded_inputs(key, cols)."""
    def make():
        n, v, gamma, _ = seeded_inputs(key, cols)
        d = sref.derive(SEED, v, gamma, IB, n)
        return [_prove_with(oracle, n, v[p], gamma[p], {k: d[k][p] for k in d}) for p in range(len(v))]
    return memo(("seeded", key, cols), make)


def accepted_proofs(oracle, key, check, max_attempts):
    """The accepted prover's CPU loop on seeded_inputs(key): per proof, attempt by attempt, try key -> scalars
    (tests/prove_try_ref.py) -> oracle.generate_range_proof -> the oracle's verifier of `check`.  Returns
    (attempts (B,) uint8, proofs): the accepted attempt's proof, the last attempt's where none was accepted
    (attempts 0), None where the value is refused (attempts 0)."""
    def make():
        n, v, gamma, _ = seeded_inputs(key)
        verify = oracle.cuda_range_proof_verify if check == 1 else oracle.range_proof_verify
        att, out = np.zeros(len(v), np.uint8), []
        for p in range(len(v)):
            kp = sref.key(SEED, v[p], gamma[p], IB + p, n)
            last = None
            for a in range(max_attempts):
                pr = _prove_with(oracle, n, v[p], gamma[p], tref.scalars(tref.try_key(kp, a), n))
                if pr is None:
                    break
                last = pr
                if verify(pr["head"], pr["V"], n, pr["a"], pr["b"], pr["L"], pr["R"], *gens(oracle, n))[0]:
                    att[p] = a + 1
                    break
            out.append(last)
        return att, out
    return memo(("accepted", key, check, max_attempts), make)


# ----------------------------------------------------------------------------- the verifier's scalar edges
V_FIELDS = ("t", "taux", "mu", "x", "c", "a[0]", "b[0]")
VN = 4


def verifier_batch(oracle):
    """synth.proofs(187, n = 4) with, for each field of V_FIELDS and each e of E, one proof whose field is e (for
    a[0] and b[0], c = <a, b> recomputed on every second one, so the fold still runs), an untouched proof after
    every third; taux and mu random.  Returns (arrays, heads, tags, want): want[p] = dict(ok, P, check, ok_std,
    det) from oracle.cuda_range_proof_verify and oracle.range_proof_verify."""
    def make():
        from cudabulletproof_amd import synth
        edits = [(f, e, j) for f in V_FIELDS for j, e in enumerate(E)]
        B = len(edits) + (len(edits) + 2) // 3
        assert B == 187
        ar = synth.proofs(B, VN, seed=2310)
        rng = np.random.default_rng(2311)
        for k in ("taux", "mu"):
            ar[k] = rng.integers(0, 2**64, size=(B, 4), dtype=np.uint64)
            ar[k][:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
        ar["Vp"] = ar["V"].copy()
        tags, p = [], 0
        for i, (f, e, j) in enumerate(edits):
            if f in ("a[0]", "b[0]"):
                ar[f[0]][p, 0] = limbs(e)
                if j % 2:
                    ar["c"][p] = oracle.inner_product(ar["a"][p], ar["b"][p])
            else:
                ar[f][p] = limbs(e)
            tags.append(("V", f, e))
            p += 1
            if i % 3 == 2 or i == len(edits) - 1:
                tags.append(("V", "untouched", None))
                p += 1
        assert p == B and sum(t[1] == "untouched" for t in tags) == 47
        heads = np.concatenate([ar[k] for k in ("Vp", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x")], axis=1)
        want = []
        for q in range(B):
            args = (heads[q], ar["V"][q], VN, ar["a"][q], ar["b"][q], ar["L"][q], ar["R"][q]) + gens(oracle, VN)
            ok, Pt, chk = oracle.cuda_range_proof_verify(*args)[:3]
            oks, det = oracle.range_proof_verify(*args)
            want.append(dict(ok=ok, P=Pt, check=chk, ok_std=oks, det=det))
        return ar, heads, tags, want
    return memo("verifier", make)


# ----------------------------------------------------------------------------- the CPU model
def canon(oracle, x):
    """The device's fe_canon / the reference's fe25519_tobytes of the four limbs of x, as an integer."""
    return memo(("canon", x), lambda: _int(oracle.fe_tobytes(limbs(x))))


def sclass(s):
    """bp_prove.hip sclass: 0 constant (zero), 1 light (<= 64 significant bits), 2 heavy."""
    return 2 if s >> 64 else (1 if s else 0)


def clz256(s):
    return 256 - s.bit_length()


def sm_ops(s):
    return (256 - clz256(s)) + bin(s).count("1")


def sm_ops_prefix(s, K):
    """ge25519_dev.h sm_ops_prefix: the chain length past the table's K bits (or past the leading zeros)."""
    if K <= 0 or clz256(s) >= K:
        return sm_ops(s)
    return (256 - K) + bin(s & ((1 << (256 - K)) - 1)).count("1")


def prefix_index(s, K):
    return s >> (256 - K)


def items(oracle, pr):
    """The scalars k_prove_prep classifies for one proof, as terms0_scalar hands them out:
    [(kind, scalar as classified, raw input)], kinds sL, sR, v, gamma (canonical), alpha, rho (raw).  The aL and
    aR terms are never queued: each is a zero-scalar constant or an entry of the per-batch table."""
    out = [("sL", canon(oracle, x), x) for x in pr["sL"]] + [("sR", canon(oracle, x), x) for x in pr["sR"]]
    out += [("v", canon(oracle, pr["v"]), pr["v"]), ("gamma", canon(oracle, pr["gamma"]), pr["gamma"])]
    out += [("alpha", pr["rnd"][0], pr["rnd"][0]), ("rho", pr["rnd"][1], pr["rnd"][1])]
    return out


def uniform_waves(oracle, proofs, K):
    """The full waves of k_prove_terms0 whose 64 lanes all hold one scalar, per scalar, under the heavy list's
    chain-length sort (longest first; the order inside a key is not defined, so only keys that a single scalar
    owns count): lane i of the launch is table lane i for i < 2n, then item i - 2n of the sorted list."""
    n = proofs[0]["n"]
    heavy = lists(oracle, proofs)["heavy"]
    by_key = {}
    for s in heavy:
        by_key.setdefault(sm_ops_prefix(s, K), []).append(s)
    out, lane = {}, 2 * n
    for key in sorted(by_key, reverse=True):
        run = by_key[key]
        if len(set(run)) == 1:
            first, last = -(-lane // 64), (lane + len(run)) // 64      # full waves inside [lane, lane + len)
            out[run[0]] = out.get(run[0], 0) + max(last - first, 0)
        lane += len(run)
    return out


def lists(oracle, proofs):
    """The terms0 work lists of a call under the model: dict(heavy=[scalars], light=[scalars],
    queued=[items queued per proof])."""
    heavy, light, queued = [], [], []
    for pr in proofs:
        q = 0
        for _, s, _ in items(oracle, pr):
            c = sclass(s)
            q += c != 0
            (heavy if c == 2 else light if c == 1 else []).append(s)
        queued.append(q)
    return dict(heavy=heavy, light=light, queued=queued)
