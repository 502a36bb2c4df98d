"""Compact proof blobs on the GPU (hipbp_batch_proof_encode / _decode, hipbp_batch_range_proof_verify_bytes_host)
against the Python restatement of the format (tests/codec_ref.py), the CPU codec and the existing
verifiers.  Inputs: the reference's 6 + 6 proofs (proofs_n16 / proofs_n64), the 28 + 16 proofs of
rpverify.npz (reference proofs, tampered copies and random limbs: accept and reject mixes, compact and
raw kinds), the n = 16 proofs tiled to 600 with copies made raw at 0, 255, 256, 257 and 599 (a raw proof
on each side of the encoder's 256-proof block boundary and at both ends), an n = 1 (no rounds) batch
and an empty one.  Only well-formed blobs reach a kernel (malformed ones: tests/codec_check.hip)."""
import os

import numpy as np
import pytest

import codec_ref as cr

pytestmark = pytest.mark.gpu
P1 = np.array([0xFFFFFFFFFFFFFFEE, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF], np.uint64)   # p + 1
RAW_AT = (0, 255, 256, 257, 599)


def _n16_all():
    """The 6 + 28 n = 16 proofs (one generator set) and the verify's V argument of each."""
    _, a, d = cr.golden_set("proofs_n16")
    _, b, r = cr.golden_set("rpverify_n16")
    arrs = {k: np.concatenate([a[k], b[k]]) for k in a}
    return arrs, np.concatenate([d["V"], r["n16_V"]]), d


def _tiled600():
    arrs, V, d = _n16_all()
    idx = np.arange(600) % len(V)
    t = cr.take(arrs, idx)
    for i in (0, 256, 599):
        t["L"][i, 0, 8:12] = P1          # Z = p + 1 in L[0], which no verifier reads: raw, same verdict
    t["b"][255, 0] = P1                  # b = 1 + p
    t["T1"][257, 15] ^= np.uint64(1)     # T off in limb 3
    return t, np.ascontiguousarray(V[idx]), d


def _n1_batch(oracle):
    """70 proofs of n = 1 (L_len = 0): random limbs, every other one made as the prover leaves a proof."""
    from cudabulletproof_amd import synth
    s = synth.proofs(70, 1, seed=11)
    rng = np.random.default_rng(5)
    arrs = {k: np.array(s[k], np.uint64) for k in cr.POINTS + ("t", "c", "x", "a", "b", "L", "R")}
    arrs["taux"] = rng.integers(0, 2**64, (70, 4), dtype=np.uint64)
    arrs["mu"] = rng.integers(0, 2**64, (70, 4), dtype=np.uint64)
    for i in range(0, 70, 2):
        for k in cr.POINTS:
            arrs[k][i, 8:12] = cr.ONE
            arrs[k][i, 12:16] = oracle.fe_mul(arrs[k][i, 0:4], arrs[k][i, 4:8])
        arrs["a"][i, 0] = arrs["c"][i] = arrs["t"][i]
        arrs["b"][i, 0] = cr.ONE
    return arrs


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> (n, arrs, the restatement's blob without and with taux / mu), computed once."""
    sets = {}
    for name in ("proofs_n16", "proofs_n64", "rpverify_n16", "rpverify_n64"):
        n, arrs, _ = cr.golden_set(name)
        sets[name] = (n, arrs)
    sets["tiled600"] = (16, _tiled600()[0])
    sets["n1"] = (1, _n1_batch(oracle))
    sets["empty"] = (64, cr.take(cr.golden_set("proofs_n64")[1], np.arange(0)))
    return {k: (n, arrs, [cr.encode(oracle, arrs, n, f) for f in (False, True)]) for k, (n, arrs) in sets.items()}


NAMES = ("proofs_n16", "proofs_n64", "rpverify_n16", "rpverify_n64", "tiled600", "n1", "empty")


def _dev():
    import torch
    return torch.device("cuda:0")


def _batch(bp, n, arrs):
    return bp.RangeProofBatch.from_numpy(n, arrs, _dev())


def _back(batch, f):
    u = lambda t: t.cpu().numpy().view(np.uint64)
    keys = cr.POINTS + ("t", "c", "x", "a", "b", "L", "R") + (("taux", "mu") if f else ())
    return {k: u(getattr(batch, k)) for k in keys}


def _blob_tensor(blob):
    import torch
    return torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(_dev())


def test_case_kinds(cases):
    """The inputs hold what the tests are about: both kinds, raw proofs where they were put."""
    n, arrs, blobs = cases["tiled600"]
    kind = np.frombuffer(blobs[0][32:32 + 600], np.uint8)
    assert all(kind[i] == 1 for i in RAW_AT) and kind[1] == 0 and kind[258] == 0 and kind[598] == 0
    assert all(0 < int(kind[b:b + 256].sum()) < len(kind[b:b + 256]) for b in (0, 256, 512))   # both kinds in every block
    kind = np.frombuffer(cases["n1"][2][1][32:32 + 70], np.uint8)
    assert list(kind) == [0, 1] * 35
    assert len(cases["empty"][2][0]) == 32


@pytest.mark.parametrize("f", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_encode_equals_restatement(bp, cases, name, f):
    n, arrs, blobs = cases[name]
    got = bp.encode_proofs(_batch(bp, n, arrs), with_blinding=f)
    assert got.numel() == len(blobs[f])   # the written size
    assert got.cpu().numpy().tobytes() == blobs[f]


@pytest.mark.parametrize("f", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_decode_returns_every_array(bp, cases, name, f):
    n, arrs, blobs = cases[name]
    batch = bp.decode_proofs(_blob_tensor(blobs[f]))   # raises unless bad = 0
    assert (batch.n, batch.count, batch.ab_len, batch.L_len) == (n, len(arrs["V"]), 1, arrs["L"].shape[1])
    assert (batch.taux is not None) == f
    got = _back(batch, f)
    assert cr.same(arrs, got, list(got))


@pytest.mark.parametrize("name", ["rpverify_n64", "tiled600", "n1"])
def test_cpu_and_gpu_codecs_cross(bp, cases, name):
    n, arrs, blobs = cases[name]
    # GPU encode -> CPU decode
    gpu_blob = bp.encode_proofs(_batch(bp, n, arrs), with_blinding=True).cpu().numpy().tobytes()
    back = cr.from_dicts(bp.proofs_from_bytes(gpu_blob), True)
    assert cr.same(arrs, back, list(arrs))
    # CPU encode -> GPU decode
    cpu_blob = bp.proofs_to_bytes(cr.to_dicts(arrs), n, with_blinding=True)
    assert cpu_blob == gpu_blob
    got = _back(bp.decode_proofs(_blob_tensor(cpu_blob)), True)
    assert cr.same(arrs, got, list(got))
    # decode(encode(x)) on the device alone, through a batch that keeps its own V apart (Vp is what is encoded)
    b = _batch(bp, n, dict(arrs, Vp=arrs["V"], V=np.zeros_like(arrs["V"])))
    got = _back(bp.decode_proofs(bp.encode_proofs(b, with_blinding=True)), True)
    assert cr.same(arrs, got, list(got))


@pytest.mark.parametrize("n", [16, 64])
def test_verify_bytes_check1_golden(bp, cases, golden, n):
    d = golden(f"proofs_n{n}")
    blob = cases[f"proofs_n{n}"][2][0]
    want = d["ok_cuda"].astype(bool)
    assert np.array_equal(bp.batch_range_proof_verify_bytes_host(blob, n, d["G"], d["H"], d["g"], d["h"]), want)
    assert np.array_equal(bp.batch_range_proof_verify_bytes_host(blob, n, d["G"], d["H"], d["g"], d["h"], V=d["V"]), want)


def test_verify_bytes_check1_600(bp, cases, monkeypatch):
    """A raw proof in each chunk position the slices can take, two verify pipelines, three shards,
    with and without the prefix tables: the struct path's verdicts."""
    arrs, V, d = _tiled600()
    blob = cases["tiled600"][2][0]
    gens = (d["G"], d["H"], d["g"], d["h"])
    want = bp.batch_range_proof_verify_host(cr.to_dicts(arrs), V, 16, *gens, num_gpus=1)
    assert want.any() and not want.all()
    got = bp.batch_range_proof_verify_bytes_host(blob, 16, *gens, V=V)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    # the proof's own V as the verify's V argument: the struct path given the same V
    own = bp.batch_range_proof_verify_host(cr.to_dicts(arrs), arrs["V"], 16, *gens, num_gpus=1)
    assert np.array_equal(bp.batch_range_proof_verify_bytes_host(blob, 16, *gens), own)
    monkeypatch.setenv("HIPBP_HOST_SHARDS", "3")
    assert np.array_equal(bp.batch_range_proof_verify_bytes_host(blob, 16, *gens, V=V, num_gpus=0), want)
    monkeypatch.delenv("HIPBP_HOST_SHARDS")
    monkeypatch.setenv("HIPBP_HOST_PREFIX_BITS", "0")
    assert np.array_equal(bp.batch_range_proof_verify_bytes_host(blob, 16, *gens, V=V), want)


@pytest.mark.parametrize("n", [16, 64])
def test_verify_bytes_check2(bp, cases, oracle, golden, n):
    d = golden("rpverify")
    blob = cases[f"rpverify_n{n}"][2][1]
    G, H = oracle.base_points(n, 1), oracle.base_points(n, 2)
    g, h = oracle.gh()
    got = bp.batch_range_proof_verify_bytes_host(blob, n, G, H, g, h, V=d[f"n{n}_V"], check=2)
    assert np.array_equal(got, d[f"n{n}_ok"].astype(bool)), np.nonzero(got != d[f"n{n}_ok"])[0]


def test_argument_errors(bp, cases, golden):
    import ctypes

    import torch
    n, arrs, blobs = cases["proofs_n16"]
    d = golden("proofs_n16")
    gens = (d["G"], d["H"], d["g"], d["h"])
    L = bp.lib()
    batch = _batch(bp, n, arrs)
    s = batch.c_struct()
    cap = L.hipbp_proof_blob_bound(6, 1, 4, 0)
    blob = torch.zeros(cap, dtype=torch.uint8, device=_dev())
    nb = torch.zeros(1, dtype=torch.int64, device=_dev())
    st = bp._stream_ptr(None)
    enc = lambda f, c: L.hipbp_batch_proof_encode(ctypes.byref(s), f, ctypes.c_void_p(blob.data_ptr()), ctypes.c_size_t(c),
                                                  ctypes.c_void_p(nb.data_ptr()), st)
    assert enc(0, cap - 1) == 1 and b"cap" in L.hipbp_last_error()           # a small cap
    s.taux = s.mu = None
    assert enc(1, cap + 4096) == 1 and b"taux" in L.hipbp_last_error()       # with_blinding without taux
    torch.cuda.synchronize()
    assert int(nb.item()) == 0 and not blob.any()                             # nothing was enqueued
    with pytest.raises(bp.BulletproofError, match="taux"):
        bp.batch_range_proof_verify_bytes_host(blobs[0], n, *gens, check=2)   # check 2 on an f = 0 blob
    with pytest.raises(bp.BulletproofError, match="header"):
        bp.batch_range_proof_verify_bytes_host(blobs[0], 32, *gens)           # n disagreeing with the header
    with pytest.raises(bp.BulletproofError, match="check"):
        bp.batch_range_proof_verify_bytes_host(blobs[0], n, *gens, check=3)


def test_verify_bytes_too_many_gpus(bp, oracle):
    """num_gpus beyond the visible devices: the code and message of every host-data entry point
    (tests/test_commit_gpu.py asserts the same of the commitments), a sentinel-filled ok untouched."""
    import ctypes

    from cudabulletproof_amd import synth
    blob = np.frombuffer(cr.encode(oracle, synth.proofs(3, 8, seed=3), 8, False), np.uint8).copy()
    G, H = (np.ascontiguousarray(oracle.base_points(8, k), np.uint64) for k in (1, 2))
    g, h = (np.ascontiguousarray(x, np.uint64) for x in oracle.gh())
    L = bp.lib()
    ndev = bp.require_gpu()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    gv, hv = bp.PointVector(p(G).value, 8), bp.PointVector(p(H).value, 8)
    ok = np.full(3, 0xA5, np.uint8)
    rc = L.hipbp_batch_range_proof_verify_bytes_host(p(blob), ctypes.c_size_t(len(blob)), None, ctypes.c_size_t(8),
                                                     ctypes.byref(gv), ctypes.byref(hv), p(g), p(h), ctypes.c_int(1),
                                                     ctypes.c_int(ndev + 1), p(ok))
    assert rc == 1 and L.hipbp_last_error().decode() == f"num_gpus = {ndev + 1} but {ndev} HIP device(s) visible"
    assert (ok == 0xA5).all()


def test_release_stream_workspaces_then_encode(bp, cases):
    import torch
    n, arrs, blobs = cases["tiled600"]
    st = torch.cuda.Stream()
    batch = _batch(bp, n, arrs)
    torch.cuda.synchronize()
    assert bp.encode_proofs(batch, with_blinding=True, stream=st).cpu().numpy().tobytes() == blobs[1]
    bp.release_stream_workspaces(st)
    assert bp.encode_proofs(batch, with_blinding=True, stream=st).cpu().numpy().tobytes() == blobs[1]
    bp.release_stream_workspaces(st)
