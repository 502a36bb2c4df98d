"""CPU checks of tests/ip_orders_ref.py, the thread-level model of the reference's inner-product
kernels (cuda_inner_product.cu:33-61, :69-92, :154-183, :219-299):

* the model and the C restatement (oracle.ip_gpu_shared / ip_gpu / ip_gpu_batch), two statements of
  the same reduction orders written from the reference's lines independently, give the same bits at
  every length the GPU tests sweep (tests/test_ref_surface_shapes_gpu.py imports the same lists);
* the live sets (which inputs reach the result), as literals;
* every mutant of the model differs from the true model at some swept length: the evidence that the
  lists reach every guard, cap and stride they are meant to.

Everything is integer arithmetic and compared with np.array_equal.
"""
import numpy as np
import pytest

import ip_orders_ref as ref


class _Env:
    def __init__(self, oracle):
        self.oracle = oracle
        self.ar = ref.Arith(oracle)
        self.a, self.b = ref.draw_inputs(ref.MAX_N)
        self.true = {}

    def run(self, kind, case, mutant=None):
        """The model's value for one swept case; the true model's are kept."""
        if mutant is None and (kind, case) in self.true:
            return self.true[kind, case]
        if kind == "shared":
            v = ref.ip_shared(self.ar, self.a, self.b, case, mutant)[0]
        elif kind == "grid":
            v = ref.ip_grid(self.ar, self.a, self.b, case, mutant)[0]
        else:
            v = ref.ip_batch(self.ar, self.a, self.b, case[0], case[1], mutant)[0]
        if mutant is None:
            self.true[kind, case] = v
        return v


@pytest.fixture(scope="module")
def env(oracle):
    return _Env(oracle)


def test_inputs_carry_the_edge_pool(env):
    """Every 64-element stretch of a and of b holds a pool element, every pool element occurs in
    both, and pool elements meet each other at one index."""
    pool = {row.tobytes() for row in ref.edge_pool()}
    for v in (env.a, env.b):
        hit = np.array([v[i].tobytes() in pool for i in range(64 * 200)])
        assert hit.reshape(200, 64).any(axis=1).all()
        assert {v[i].tobytes() for i in np.flatnonzero(hit)} == pool
    both = [i for i in range(64 * 200) if env.a[i].tobytes() in pool and env.b[i].tobytes() in pool]
    assert len(both) >= 60
    top = env.a[:, 3] >> np.uint64(63)
    assert 0.4 < top[:4096].mean() < 0.6   # full 256-bit limbs, not masked ones


def test_shared_model_matches_oracle(env):
    a, b = env.a, env.b
    bad = [n for n in ref.SHARED_ENTRY_N
           if not np.array_equal(env.run("shared", n), env.oracle.ip_gpu(a[:n], b[:n], shared=True))]
    assert not bad, bad
    # cuda_field_vector_inner_product takes the same kernel up to 512 (:108-111)
    bad = [n for n in (1, 2, 3, 66, 511, 512)
           if not np.array_equal(ref.ip_grid(env.ar, a, b, n)[0], env.oracle.ip_gpu(a[:n], b[:n]))]
    assert not bad, bad


def test_grid_model_matches_oracle(env):
    a, b = env.a, env.b
    bad = [n for n in ref.GRID_N if not np.array_equal(env.run("grid", n), env.oracle.ip_gpu(a[:n], b[:n]))]
    assert not bad, bad


def test_batch_model_matches_oracle(env):
    bad = []
    for n, nv in ref.BATCH_CASES:
        want = env.oracle.ip_gpu_batch(env.a[:n * nv].reshape(nv, n, 4), env.b[:n * nv].reshape(nv, n, 4))
        if not np.array_equal(env.run("batch", (n, nv)), want):
            bad.append((n, nv))
    assert not bad, bad


def test_live_sets(env):
    a, b = env.a, env.b
    live = lambda f, *args: f(None, a, b, *args)[1]
    assert live(ref.ip_shared, 1).tolist() == [0]
    assert live(ref.ip_shared, 2).tolist() == [0, 1]
    assert live(ref.ip_shared, 3).tolist() == [0, 1]             # blockDim 3: the tree starts at 1
    assert live(ref.ip_shared, 6).tolist() == [0, 1, 3, 4]       # strides 3, 1
    assert live(ref.ip_shared, 7).tolist() == [0, 1, 3, 4]
    assert live(ref.ip_shared, 66).tolist() == list(range(32)) + list(range(33, 65))   # strides 33, 16, .., 1
    assert live(ref.ip_shared, 512).tolist() == list(range(512))
    assert live(ref.ip_shared, 513).tolist() == list(range(512))  # 512 is dead: one block of 512 threads
    assert live(ref.ip_shared, 5000).tolist() == list(range(512))
    assert live(ref.ip_grid, 512).tolist() == list(range(512))
    assert live(ref.ip_grid, 513).tolist() == list(range(513))
    assert np.array_equal(live(ref.ip_grid, 65536), np.arange(65536))
    assert np.array_equal(live(ref.ip_grid, 70000), np.arange(65536))   # blocks 256.. are unread
    lv = live(ref.ip_grid, 262144)
    assert np.array_equal(lv, np.arange(65536))
    lv = live(ref.ip_grid, 262145)
    assert np.array_equal(lv, np.append(np.arange(65536), 262144))      # block 0's second turn
    lv = live(ref.ip_grid, 3 * 262144 + 77)
    assert len(lv) == 3 * 65536 + 77 and lv[-1] == 3 * 262144 + 76
    assert live(ref.ip_batch, 256, 1).tolist() == list(range(256))
    assert live(ref.ip_batch, 257, 1).tolist() == list(range(256))      # 256 is dead: x-block 1's
    assert live(ref.ip_batch, 1000, 3).tolist() == list(range(256))
    assert live(ref.ip_batch, 262144 + 259, 2).tolist() == list(range(256)) + list(range(262144, 262144 + 256))


def test_model_refuses_a_race():
    s = ref._Lds(4, None)
    for t in range(3):
        s.zero(t)
    with pytest.raises(ref.ModelError):
        s.add_phase([(0, 1), (1, 2)])     # thread 0 reads what thread 1 writes
    with pytest.raises(ref.ModelError):
        s.add_phase([(0, 3)])             # slot 3 was never written
    s.add_phase([(0, 2), (1, 2)])


def _cases():
    for n in ref.DISPATCH_N:
        yield "grid", n
    for n in ref.SHARED_GPU_N:
        yield "shared", n
    for c in ref.BATCH_CASES:
        yield "batch", c
    for n in ref.GRID_N:
        yield "grid", n


def _first_difference(env, mutant):
    for kind, case in _cases():
        if not np.array_equal(env.run(kind, case, mutant), env.run(kind, case)):
            return kind, case
    return None


@pytest.mark.parametrize("mutant", sorted(set(ref.MUTANTS) - set(ref.EQUIVALENT_MUTANTS)))
def test_shape_lists_tell_every_mutant_apart(env, mutant):
    """At least one case of the lists the GPU tests sweep gives the mutant other bits than the true
    model.  (A mutant no case catches means a shape is missing from a list.)"""
    assert _first_difference(env, mutant) is not None, \
        f"no swept shape tells '{mutant}' ({ref.MUTANTS[mutant]}) from the true model"


@pytest.mark.parametrize("mutant", ref.EQUIVALENT_MUTANTS)
def test_guard_mutants_are_equivalent_in_the_wrappers_shapes(env, mutant):
    """The two guard mutants cannot be told apart by any length: in the shapes the reference's
    wrappers launch, its `tid + stride < n` guards never keep a live value out (the argument is at
    ip_orders_ref.EQUIVALENT_MUTANTS).  Pinned here instead: the shared tree's guard never fails at
    any n, the reduce's guard only ever skips zeroed slots (same live sets, same bits over every
    swept case), and the mutants are real: one launch outside the wrappers' shapes separates them."""
    for n in range(1, 1100):
        st = min(n, ref.MAX_SHARED_ELEMENTS) // 2
        while st:
            assert (st - 1) + st < n          # the largest tid + stride of the phase
            st >>= 1
    for n in (513, 768, 1279, 9472, 17920, 65243, 65536, 65755):   # 3 .. 257 partials
        assert n in ref.GRID_N
        assert np.array_equal(ref.ip_grid(None, env.a, env.b, n, mutant)[1], ref.ip_grid(None, env.a, env.b, n)[1])
    assert _first_difference(env, mutant) is None
    one, top = ref.fe_int(1)[None].copy(), ref.fe_int(2**256 - 1)[None].copy()
    ar = ref.Arith(env.oracle)
    true = ref.shared_kernel(ar, one, top, 1, 2)[0]
    assert np.array_equal(true, ref.fe_int(2**255 + 18))          # a product >= p, as fe25519_mul leaves it
    got = ref.shared_kernel(ar, one, top, 1, 2, mutant)[0]        # ... and adding slot 1's zero changes it
    assert np.array_equal(got, env.oracle.fe_add(true, ref.fe_int(0))) and not np.array_equal(got, true)
