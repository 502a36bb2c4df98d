"""Proof ids and the batch Merkle root on the GPU (hipbp_batch_proof_ids, hipbp_blob_proof_ids,
hipbp_merkle_root) against the Python restatement (tests/proof_id_ref.py) and the CPU
paths.  Inputs, rebuilt here from codec_ref: the reference's 6 + 6 proofs, the 28 + 16 proofs of
rpverify.npz (compact and raw kinds), the n = 16 proofs tiled to 600 with copies made raw at 0, 255, 256,
257 and 599 (both sides of a 256-lane block, a ragged last wave), an n = 1 (no rounds) batch, an empty
one and an ab_len = 2 batch (every proof raw).  Only well-formed blobs reach a kernel (malformed ones:
tests/ids_check.hip).  The tree is one launch per level at every size: no size changes its path."""
import ctypes

import numpy as np
import pytest

import codec_ref as cr
import proof_id_ref as pr

pytestmark = pytest.mark.gpu
P1 = np.array([0xFFFFFFFFFFFFFFEE, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF], np.uint64)   # p + 1
RAW_AT = (0, 255, 256, 257, 599)
NAMES = ("proofs_n16", "proofs_n64", "rpverify_n16", "rpverify_n64", "tiled600", "n1", "empty", "ab2")


def _tiled600():
    _, a, _ = cr.golden_set("proofs_n16")
    _, b, _ = cr.golden_set("rpverify_n16")
    arrs = {k: np.concatenate([a[k], b[k]]) for k in a}
    t = cr.take(arrs, np.arange(600) % len(arrs["V"]))
    for i in (0, 256, 599):
        t["L"][i, 0, 8:12] = P1          # Z = p + 1 in L[0]
    t["b"][255, 0] = P1                  # b = 1 + p
    t["T1"][257, 15] ^= np.uint64(1)     # T off in limb 3
    return t


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


def _ab2():
    _, arrs, _ = cr.golden_set("proofs_n16")
    two = dict(arrs)
    two["a"] = np.concatenate([arrs["a"], arrs["a"] + np.uint64(1)], axis=1)
    two["b"] = np.concatenate([arrs["b"], arrs["b"] + np.uint64(2)], axis=1)
    return two


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> (n, arrs, [(ids, kinds) of the restatement without and with taux / mu]), computed once."""
    sets = {}
    for name in ("proofs_n16", "proofs_n64", "rpverify_n16", "rpverify_n64"):
        n, arrs, _ = cr.golden_set(name)
        sets[name] = (n, arrs)
    sets["tiled600"] = (16, _tiled600())
    sets["n1"] = (1, _n1_batch(oracle))
    sets["empty"] = (64, cr.take(cr.golden_set("proofs_n64")[1], np.arange(0)))
    sets["ab2"] = (16, _ab2())
    return {k: (n, arrs, [pr.proof_ids(oracle, arrs, n, f) for f in (False, True)]) for k, (n, arrs) in sets.items()}


def _dev():
    import torch
    return torch.device("cuda:0")


def _batch(bp, n, arrs):
    return bp.RangeProofBatch.from_numpy(n, arrs, _dev())


def _ids(t):
    a = t.cpu().numpy()
    return [a[i].tobytes() for i in range(len(a))]


def test_case_kinds(cases):
    """The inputs hold what the tests are about: both kinds, raw proofs where they were put."""
    kinds = cases["tiled600"][2][0][1]
    assert all(kinds[i] == 1 for i in RAW_AT) and kinds[1] == 0 and kinds[258] == 0 and kinds[598] == 0
    assert all(0 < sum(kinds[b:b + 256]) < len(kinds[b:b + 256]) for b in (0, 256, 512))
    assert cases["n1"][2][1][1] == [0, 1] * 35
    assert cases["ab2"][2][0][1] == [1] * 6 and cases["empty"][2][0] == ([], [])
    assert 0 < sum(cases["rpverify_n64"][2][1][1]) < 16


@pytest.mark.parametrize("f", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_proof_ids_equal_restatement(bp, cases, name, f):
    n, arrs, want = cases[name]
    ids, kinds = bp.proof_ids(_batch(bp, n, arrs), with_blinding=f, return_kinds=True)
    assert tuple(ids.shape) == (len(arrs["V"]), 32)
    assert list(kinds.cpu().numpy()) == want[f][1]
    got = _ids(ids)
    bad = [i for i in range(len(got)) if got[i] != want[f][0][i]]
    assert not bad, bad[:10]
    assert _ids(bp.proof_ids(_batch(bp, n, arrs), with_blinding=f)) == want[f][0]   # without kind_dev


@pytest.mark.parametrize("f", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_blob_ids_equal_batch_ids(bp, cases, name, f):
    n, arrs, want = cases[name]
    batch = _batch(bp, n, arrs)
    ids, bad = bp.blob_proof_ids(bp.encode_proofs(batch, with_blinding=f))
    assert int(bad.item()) == 0
    assert _ids(ids) == want[f][0]
    assert (ids == bp.proof_ids(batch, with_blinding=f)).all()


@pytest.mark.parametrize("name", ["rpverify_n16", "rpverify_n64", "tiled600", "n1", "ab2"])
def test_gpu_ids_equal_host_ids(bp, cases, name):
    n, arrs, want = cases[name]
    host = bp.proof_ids_host(cr.to_dicts(arrs), n, True)
    assert _ids(bp.proof_ids(_batch(bp, n, arrs), with_blinding=True)) == host
    blob = bp.proofs_to_bytes(cr.to_dicts(arrs), n, with_blinding=True)
    assert bp.blob_proof_ids_host(blob) == host
    # a batch that keeps its own V apart: Vp is what is hashed, as it is what is encoded
    b = _batch(bp, n, dict(arrs, Vp=arrs["V"], V=np.zeros_like(arrs["V"])))
    assert _ids(bp.proof_ids(b, with_blinding=True)) == host


# one launch per level at every size: 255 / 256 / 257 and 600 put level 1 on both sides of a block
COUNTS = (0, 1, 2, 3, 255, 256, 257, 511, 512, 513, 600, 4097)


@pytest.fixture(scope="module")
def roots():
    ids = pr.kat_ids(4097)
    return ids, {c: pr.mth(ids[:c]) for c in COUNTS}


@pytest.mark.parametrize("count", COUNTS)
def test_merkle_root_equals_restatement(bp, roots, count):
    import torch
    ids, want = roots
    t = torch.from_numpy(pr.ids_array(ids[:count]).copy()).to(_dev())
    root = bp.merkle_root(t)
    assert root.cpu().numpy().tobytes() == want[count]
    assert bp.merkle_root_host(ids[:count]) == want[count]


def test_root_of_a_batch(bp, cases):
    """ids and root without leaving the device: the restatement's root over its ids."""
    n, arrs, want = cases["tiled600"]
    root = bp.merkle_root(bp.proof_ids(_batch(bp, n, arrs), with_blinding=True))
    assert root.cpu().numpy().tobytes() == pr.mth(want[1][0])


def test_argument_errors(bp, cases):
    import torch
    n, arrs, want = cases["proofs_n16"]
    L = bp.lib()
    batch = _batch(bp, n, arrs)
    s = batch.c_struct()
    st = bp._stream_ptr(None)
    ids = torch.zeros(6, 32, dtype=torch.uint8, device=_dev())
    kinds = torch.full((6,), 9, dtype=torch.uint8, device=_dev())
    call = lambda f, p=None: L.hipbp_batch_proof_ids(ctypes.byref(s), f, ctypes.c_void_p(p if p is not None else ids.data_ptr()),
                                                     ctypes.c_void_p(kinds.data_ptr()), st)
    s.taux = s.mu = None
    assert call(1) == 1 and b"taux" in L.hipbp_last_error()          # with_blinding without taux
    assert call(0, 0) == 1 and b"null" in L.hipbp_last_error()       # null ids
    s.n = 24
    assert call(0) == 1 and b"power of two" in L.hipbp_last_error()  # a bad shape
    s.n = n
    s.A = None
    assert call(0) == 1 and b"null batch field" in L.hipbp_last_error()
    s = batch.c_struct()
    root = torch.zeros(32, dtype=torch.uint8, device=_dev())
    assert L.hipbp_merkle_root(ctypes.c_void_p(ids.data_ptr()), ctypes.c_size_t((1 << 24) + 1), ctypes.c_void_p(root.data_ptr()), st) == 1
    assert b"2^24" in L.hipbp_last_error()
    assert L.hipbp_merkle_root(None, ctypes.c_size_t(6), ctypes.c_void_p(root.data_ptr()), st) == 1
    assert L.hipbp_merkle_root(ctypes.c_void_p(ids.data_ptr()), ctypes.c_size_t(6), None, st) == 1
    blob = bp.encode_proofs(batch)
    ic = bp.ProofBlobInfoC()
    head = blob[:32].cpu().numpy()
    assert L.hipbp_proof_blob_header(bp._p(head), ctypes.c_size_t(blob.numel()), ctypes.byref(ic)) == 0
    badw = torch.full((1,), 7, dtype=torch.int32, device=_dev())
    ic.bytes += 8                                                   # an info that describes no blob
    assert L.hipbp_blob_proof_ids(ctypes.c_void_p(blob.data_ptr()), ctypes.byref(ic), ctypes.c_void_p(ids.data_ptr()),
                                  ctypes.c_void_p(badw.data_ptr()), st) == 1 and b"info" in L.hipbp_last_error()
    ic.bytes -= 8
    assert L.hipbp_blob_proof_ids(None, ctypes.byref(ic), ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(badw.data_ptr()), st) == 1
    torch.cuda.synchronize()
    # nothing was enqueued
    assert not ids.any() and (kinds == 9).all() and not root.any() and int(badw.item()) == 7
    assert call(0) == 0
    torch.cuda.synchronize()
    assert _ids(ids) == want[0][0] and not kinds.any()


def test_release_stream_workspaces_then_root(bp, cases, roots):
    import torch
    ids, want = roots
    n, arrs, w = cases["tiled600"]
    st = torch.cuda.Stream()
    batch = _batch(bp, n, arrs)
    t = torch.from_numpy(pr.ids_array(ids[:600]).copy()).to(_dev())
    blob = bp.encode_proofs(batch, with_blinding=True)
    torch.cuda.synchronize()
    for _ in range(2):
        root = bp.merkle_root(t, stream=st)
        bids, bad = bp.blob_proof_ids(blob, stream=st)
        st.synchronize()
        assert root.cpu().numpy().tobytes() == want[600]
        assert int(bad.item()) == 0 and _ids(bids) == w[1][0]
        bp.release_stream_workspaces(st)
    # a small tree, then a larger one on the same stream: the workspace grows under queued work
    r3 = bp.merkle_root(t[:3], stream=st)
    r600 = bp.merkle_root(t, stream=st)
    st.synchronize()
    assert r3.cpu().numpy().tobytes() == want[3] and r600.cpu().numpy().tobytes() == want[600]
    bp.release_stream_workspaces(st)
