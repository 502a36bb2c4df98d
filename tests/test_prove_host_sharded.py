"""The provers on host structs: batch_generate_range_proof_accepted_host against the device
call batch_generate_range_proof_accepted (which tests/test_prove_accepted.py pins to the CPU oracle)
and against the oracle's attempts as literals; batch_generate_range_proof_host split into shards
against its one-device form; the call's statistics, max_attempts = 2, both checks at n = 64, the
argument errors, and two real devices where there are two.  The shards run as virtual shards
(HIPBP_HOST_SHARDS) on one device, so the split, its threads and the merge are covered on a one-GPU
machine; the chunk rules are reached with HIPBP_PROVE_HOST_ACCEPT_CHUNK / HIPBP_PROVE_HOST_CHUNK."""
import ctypes

import numpy as np
import pytest

from test_prove_seeded import KEYS, SEED, inputs

pytestmark = pytest.mark.gpu

IB = 7
HEAD = ("V", "A", "S", "T1", "T2", "taux", "mu", "t", "c", "x")

# n = 8, B = 70, default_rng(10), proof 17 refused, index_base 7, check 1: the CPU oracle's attempts
WANT8 = np.ones(70, np.uint8)
WANT8[[4, 56]] = 3
WANT8[[19, 29, 30, 35, 36, 61]] = 2
WANT8[17] = 0


@pytest.fixture(scope="module")
def T():
    import torch
    dev = torch.device("cuda:0")
    return lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(dev)


@pytest.fixture(scope="module")
def gens_for(oracle):
    cache = {}

    def get(n):
        if n not in cache:
            g, h = oracle.gh()
            cache[n] = (oracle.base_points(n, 1), oracle.base_points(n, 2), g, h)
        return cache[n]
    return get


@pytest.fixture(scope="module")
def device_call(bp, T, gens_for):
    """batch_generate_range_proof_accepted's output as numpy arrays, computed once per case."""
    cache = {}

    def get(n, v, gamma, max_attempts=8, check=1):
        import torch
        key = (n, v.tobytes(), max_attempts, check)
        if key not in cache:
            G, H, g, h = (T(x) for x in gens_for(n))
            o = bp.batch_generate_range_proof_accepted(n, T(v), T(gamma), SEED, G, H, g, h, index_base=IB,
                                                       max_attempts=max_attempts, check=check)
            torch.cuda.synchronize()
            cache[key] = {k: o[k].cpu().numpy() if k in ("valid", "attempts") else o[k].cpu().numpy().view(np.uint64)
                          for k in KEYS + ("attempts",)}
        return cache[key]
    return get


def case8():
    return (8, 70) + inputs(70, 8, np.random.default_rng(10), refuse=17)


def structs_equal_rows(proofs, valid, d, n):
    """Every proof dict equals the device tensors' row: head, a, b, L, R, n and L_len; a refused value
    has the zero ip_proof (n = L_len = 0, empty vectors, c = x = 0)."""
    Lr = n.bit_length() - 1
    assert len(proofs) == len(d["valid"]) and np.array_equal(valid, d["valid"].astype(bool))
    for p, pr in enumerate(proofs):
        head = np.concatenate([d[k][p] for k in HEAD])
        if valid[p]:
            assert np.array_equal(pr["head"], head), p
            assert pr["n"] == n and pr["L_len"] == Lr, p
            for k in ("a", "b", "L", "R"):
                assert np.array_equal(pr[k], d[k][p].reshape(pr[k].shape)), (p, k)
        else:
            assert np.array_equal(pr["head"][:92], head[:92]), p
            assert not pr["head"][92:].any() and pr["n"] == 0 and pr["L_len"] == 0, p
            assert all(len(pr[k]) == 0 for k in ("a", "b", "L", "R")), p


def set_env(monkeypatch, shards=None, accept_chunk=None, chunk=None):
    for name, val in (("HIPBP_HOST_SHARDS", shards), ("HIPBP_PROVE_HOST_ACCEPT_CHUNK", accept_chunk),
                      ("HIPBP_PROVE_HOST_CHUNK", chunk)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))


@pytest.mark.parametrize("accept_chunk", [None, 16])
@pytest.mark.parametrize("shards", [None, 3])
def test_accepted_host_equals_device_call(bp, gens_for, device_call, monkeypatch, shards, accept_chunk):
    """n = 8, B = 70, default_rng(10), proof 17 refused, index_base 7, check 1, max_attempts 8.  Three
    shards are the blocks [0,23), [23,46), [46,70): each holds a retry (4 and 19; 29, 30, 35 and 36; 56
    and 61) and shard 0 the refused value; with chunk 16 a shard spans two chunks.  attempts equals the
    device call's and the oracle's literals, valid the device call's, every struct its row of the
    device tensors; batch_range_proof_verify_host accepts exactly the proofs with attempts > 0."""
    n, B, v, gamma = case8()
    d = device_call(n, v, gamma)
    set_env(monkeypatch, shards=shards, accept_chunk=accept_chunk)
    Gn, Hn, gn, hn = gens_for(n)
    proofs, valid, attempts = bp.batch_generate_range_proof_accepted_host(v, gamma, n, Gn, Hn, gn, hn, SEED, index_base=IB,
                                                                         max_attempts=8, check=1, num_gpus=0)
    assert attempts.dtype == np.uint8 and np.array_equal(attempts, d["attempts"]) and np.array_equal(attempts, WANT8)
    assert valid.tolist() == [p != 17 for p in range(B)]
    structs_equal_rows(proofs, valid, d, n)
    V = np.stack([pr["head"][:16] for pr in proofs])
    ok = bp.batch_range_proof_verify_host(proofs, V, n, Gn, Hn, gn, hn, num_gpus=1)
    assert np.array_equal(ok[valid], attempts[valid] > 0) and ok[valid].all()


@pytest.mark.parametrize("accept_chunk", [None, 16])
@pytest.mark.parametrize("shards", [None, 3])
def test_stats_report_the_whole_call(bp, gens_for, monkeypatch, shards, accept_chunk):
    """accepted_last_stats after the host call: the largest round count of any chunk and the proofs
    proved per round summed over all shards and chunks (the device calls run on the shards' threads)."""
    n, B, v, gamma = case8()
    set_env(monkeypatch, shards=shards, accept_chunk=accept_chunk)
    Gn, Hn, gn, hn = gens_for(n)
    bp.batch_generate_range_proof_accepted_host(v, gamma, n, Gn, Hn, gn, hn, SEED, index_base=IB, num_gpus=0)
    st = bp.accepted_last_stats()
    assert st["rounds"] == 3 and st["proved"] == [70, 8, 2], st


@pytest.mark.parametrize("shards", [None, 3])
def test_two_attempts_keep_the_last_proof(bp, gens_for, device_call, monkeypatch, shards):
    """max_attempts = 2: proofs 4 and 56 end with attempts 0 and valid True and hold the device call's
    last-attempt proof; the rest as with 8 attempts.  Unsharded (num_gpus = 1) and in three shards."""
    n, B, v, gamma = case8()
    d = device_call(n, v, gamma, max_attempts=2)
    set_env(monkeypatch, shards=shards)
    Gn, Hn, gn, hn = gens_for(n)
    proofs, valid, attempts = bp.batch_generate_range_proof_accepted_host(
        v, gamma, n, Gn, Hn, gn, hn, SEED, index_base=IB, max_attempts=2, num_gpus=1 if shards is None else 0)
    assert np.array_equal(attempts, np.where(WANT8 <= 2, WANT8, 0)) and np.array_equal(attempts, d["attempts"])
    assert attempts[4] == 0 and attempts[56] == 0 and valid[4] and valid[56]
    structs_equal_rows(proofs, valid, d, n)


@pytest.mark.parametrize("check", [1, 2])
def test_n64_both_checks(bp, gens_for, device_call, monkeypatch, check):
    """n = 64, B = 24, default_rng(566), two shards: the device call's results under both checks; the
    oracle's second attempt at proof 14 (check 1, shard 1) and at proof 9 (check 2, shard 0)."""
    n, B = 64, 24
    v, gamma = inputs(B, n, np.random.default_rng(566))
    d = device_call(n, v, gamma, check=check)
    set_env(monkeypatch, shards=2)
    Gn, Hn, gn, hn = gens_for(n)
    proofs, valid, attempts = bp.batch_generate_range_proof_accepted_host(v, gamma, n, Gn, Hn, gn, hn, SEED, index_base=IB,
                                                                         check=check, num_gpus=0)
    want = np.ones(B, np.uint8)
    want[14 if check == 1 else 9] = 2
    assert np.array_equal(attempts, want) and np.array_equal(attempts, d["attempts"]) and valid.all()
    structs_equal_rows(proofs, valid, d, n)


def same_proofs(a, b):
    (pa, va), (pb, vb) = a, b
    assert np.array_equal(va, vb) and len(pa) == len(pb)
    for p, (x, y) in enumerate(zip(pa, pb)):
        assert x["n"] == y["n"] and x["L_len"] == y["L_len"], p
        for k in ("head", "a", "b", "L", "R"):
            assert x[k].shape == y[k].shape and np.array_equal(x[k], y[k]), (p, k)


@pytest.mark.parametrize("index_base", [2**32 - 3, 2**64 - 2])
def test_seeded_host_sharded(bp, gens_for, monkeypatch, index_base):
    """The existing host test's case (n = 16, count = 9, proof 5 refused, default_rng(16)) in three
    shards, and again with chunks of 2 inside them, is byte-identical to num_gpus = 1; at index_base
    2^64 - 2 the index wraps inside shard 0."""
    n, B = 16, 9
    v, gamma = inputs(B, n, np.random.default_rng(16), refuse=5)
    gens = gens_for(n)
    set_env(monkeypatch)
    one = bp.batch_generate_range_proof_host(v, gamma, n, *gens, SEED, index_base=index_base, num_gpus=1)
    assert one[1].sum() == B - 1 and not one[1][5] and all(pr["L_len"] == 4 for p, pr in enumerate(one[0]) if p != 5)
    set_env(monkeypatch, shards=3)
    same_proofs(bp.batch_generate_range_proof_host(v, gamma, n, *gens, SEED, index_base=index_base, num_gpus=0), one)
    set_env(monkeypatch, shards=3, chunk=2)
    same_proofs(bp.batch_generate_range_proof_host(v, gamma, n, *gens, SEED, index_base=index_base, num_gpus=0), one)
    if index_base == 2**64 - 2:   # the wrap is real: proof 2 has index 0, as a call that starts there
        lo = bp.batch_generate_range_proof_host(v[2:], gamma[2:], n, *gens, SEED, index_base=0, num_gpus=1)
        same_proofs((one[0][2:], one[1][2:]), lo)


def test_argument_errors_write_nothing(bp, gens_for, monkeypatch):
    """num_gpus beyond the visible devices raises with the verifier's message; max_attempts 0 and 17,
    check 3, a null attempts and G of length n / 2 give HIPBP_ERR_ARG through the raw ABI and leave
    sentinel-filled proofs, valid and attempts untouched; a 31-byte seed raises in the wrapper;
    count = 0 returns HIPBP_OK."""
    set_env(monkeypatch)
    n, B = 8, 4
    v, gamma = inputs(B, n, np.random.default_rng(1))
    Gn, Hn, gn, hn = gens_for(n)
    ndev = bp.require_gpu()
    for call in (lambda: bp.batch_generate_range_proof_accepted_host(v, gamma, n, Gn, Hn, gn, hn, SEED, num_gpus=ndev + 1),
                 lambda: bp.batch_generate_range_proof_host(v, gamma, n, Gn, Hn, gn, hn, SEED, num_gpus=ndev + 1)):
        with pytest.raises(bp.BulletproofError, match=rf"num_gpus = {ndev + 1} but {ndev} HIP device"):
            call()
    with pytest.raises(ValueError):
        bp.batch_generate_range_proof_accepted_host(v, gamma, n, Gn, Hn, gn, hn, SEED[:31])
    with pytest.raises(bp.BulletproofError):
        bp.batch_generate_range_proof_accepted_host(v, gamma, n, Gn, Hn, gn, hn, SEED, max_attempts=0)

    L = bp.lib()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    u = lambda a: np.ascontiguousarray(a, np.uint64)
    vv, gg, G, H, g, h = u(v), u(gamma), u(Gn), u(Hn), u(gn), u(hn)
    sd = (ctypes.c_uint8 * 32).from_buffer_copy(SEED)

    def raw(max_attempts=8, check=1, attempts=True, glen=n, count=B, num_gpus=1, sharded=False):
        arr = (bp.RangeProofC * B)()
        ctypes.memset(arr, 0x5A, ctypes.sizeof(arr))
        valid, att = np.full(B, 0x5A, np.uint8), np.full(B, 0x5A, np.uint8)
        gv, hv = bp.PointVector(p(G).value, glen), bp.PointVector(p(H).value, n)
        head = (arr, p(valid))
        tail = (p(vv), p(gg), ctypes.c_size_t(count), ctypes.c_size_t(n), ctypes.byref(gv), ctypes.byref(hv), p(g), p(h), sd,
                ctypes.c_uint64(0))
        if sharded:
            rc = L.hipbp_batch_generate_range_proof_host_sharded(*head, *tail, ctypes.c_int(num_gpus))
        else:
            rc = L.hipbp_batch_generate_range_proof_accepted_host(*head, p(att) if attempts else None, *tail,
                                                                  ctypes.c_int(max_attempts), ctypes.c_int(check),
                                                                  ctypes.c_int(num_gpus))
        assert bytes(arr) == b"\x5a" * ctypes.sizeof(arr)
        assert (valid == 0x5A).all() and (att == 0x5A).all()
        return rc

    assert raw(max_attempts=0) == 1   # HIPBP_ERR_ARG
    assert raw(max_attempts=17) == 1
    assert raw(check=3) == 1
    assert raw(attempts=False) == 1
    assert raw(glen=n // 2) == 1
    assert raw(num_gpus=ndev + 1) == 1
    assert raw(glen=n // 2, sharded=True) == 1
    assert raw(num_gpus=ndev + 1, sharded=True) == 1
    assert raw(count=0) == 0          # HIPBP_OK, nothing written
    assert raw(count=0, sharded=True) == 0


def test_two_real_devices(bp, gens_for, device_call, monkeypatch):
    """With at least two devices visible: the accepted case and the seeded case at num_gpus = 2 equal
    num_gpus = 1."""
    if bp.require_gpu() < 2:
        pytest.skip("needs two HIP devices")
    set_env(monkeypatch)
    n, B, v, gamma = case8()
    gens = gens_for(n)
    one = bp.batch_generate_range_proof_accepted_host(v, gamma, n, *gens, SEED, index_base=IB, num_gpus=1)
    two = bp.batch_generate_range_proof_accepted_host(v, gamma, n, *gens, SEED, index_base=IB, num_gpus=2)
    st = bp.accepted_last_stats()
    same_proofs(two[:2], one[:2])
    assert np.array_equal(two[2], one[2]) and np.array_equal(two[2], WANT8)
    assert st["rounds"] == 3 and st["proved"] == [70, 8, 2], st
    n, B = 16, 9
    v, gamma = inputs(B, n, np.random.default_rng(16), refuse=5)
    gens = gens_for(n)
    for ib in (2**32 - 3, 2**64 - 2):
        same_proofs(bp.batch_generate_range_proof_host(v, gamma, n, *gens, SEED, index_base=ib, num_gpus=2),
                    bp.batch_generate_range_proof_host(v, gamma, n, *gens, SEED, index_base=ib, num_gpus=1))
