"""A thread-level model of the reference's four inner-product kernels — TEST INFRASTRUCTURE ONLY.

Written from the reference's cuda_inner_product.cu alone, one function per kernel and per wrapper:

  :33-61    field_vector_inner_product_kernel          grid_kernel_block(warp_tail=False)
  :69-92    fe25519_reduce_kernel                      reduce_kernel
  :97-151   cuda_field_vector_inner_product            ip_grid   (its launch arithmetic, :108, :123-124)
  :154-183  field_vector_inner_product_shared_kernel   shared_kernel
  :185-216  cuda_field_vector_inner_product_shared     ip_shared (:204: min(n, 512) threads)
  :219-257  warp_reduce_field_element                  warp_reduce (five lockstep `if (lane < k)` steps)
  :260-299  batch_inner_product_kernel                 grid_kernel_block(warp_tail=True)
  :302-347  cuda_batch_field_vector_inner_product      ip_batch  (:306 n = vector 0's length, :332 grid)

It is a second statement of the reduction orders next to oracle/bp_oracle.c's (orc_ip_gpu*), and
deliberately of another shape: each kernel is what its threads do between two barriers.  A phase is
a list of (tid, source slot) pairs, one per thread whose `if` holds; `_Lds.add_phase` first checks
that no thread reads a slot that was never written and that no thread reads a slot another thread of
the same phase writes (so the phase has one outcome whatever the order of the warps), then applies
the adds.  blockDim and gridDim are parameters of the kernels; only the wrappers compute them.

Element arithmetic is the oracle's fe_mul / fe_add (pinned by field.npz), called by address on rows
of uint64 arrays.  With arith=None no arithmetic is done and only the live sets are computed.

Every entry point returns (value, live): `live` is the sorted array of input indices whose products
reach the result, tracked as index sets next to the values.

The batched wrapper launches gridDim.x = min(1024, ceil(n / 256)) blocks per vector that all write
results[batch_id] (:297): a race when n > 256.  The project returns x-block 0's value, and so does
ip_batch.

`mutant=` selects ONE wrong variant (MUTANTS); tests/test_ip_orders_ref.py shows that the lengths
the GPU tests sweep tell each of them from the true model.
"""
import ctypes

import numpy as np

BLOCK_SIZE = 256            # :10
WARP_SIZE = 32              # :11
MAX_SHARED_ELEMENTS = 512   # :12
MAX_BLOCKS = 1024           # :124, :332

MUTANTS = {
    "guard_le": "the trees' guard `tid + stride < n` (:84, :172) written `tid + stride <= n`",
    "guard_none": "the trees' guard `tid + stride < n` (:84, :172) dropped",
    "tree_ceil": "the shared tree (:171) started at ceil(blockDim / 2)",
    "tree_pow2": "the shared tree (:171) run over the next power of two >= blockDim",
    "cap_1023": "the block cap (:124, :332) at 1023",
    "cap_none": "no block cap (:124, :332)",
    "reduce_255": "the reduce (:69-92) as a 255-slot block: partial 255 unread",
    "reduce_257": "the reduce (:69-92) as a 257-slot block with a tree from 256: partial 256 read",
    "reduce_all": "the reduce (:69-92) over every partial (slots and tree sized by the block count)",
    "batch_stride_block": "the batch kernel's stride (:283) blockDim.x instead of gridDim.x * blockDim.x",
    "one_turn": "the grid-stride loops (:46-51, :279-284) left after their first turn",
}


# Mutants that no launch shape of the reference's wrappers can tell from the true model, and why.
# The shared wrapper launches blockDim = min(n, 512) (:204), and the tree's strides are at most
# blockDim / 2, so tid + stride <= 2 * stride - 1 < blockDim <= n: the guard at :172 never fails.
# The reduce kernel's guard (:84) fails only for slots that :78 zeroed, and fe25519_add(x, 0) is x
# for every x < p; a partial is the last of at least eight fe25519_add results whose operands are
# themselves sums from 0 over one turn (the guard is reachable only below 256 blocks, where no thread
# takes a second turn), and those are below p.  The guards matter as soon as a kernel runs in a
# shape the wrappers never launch: shared_kernel with blockDim 2 and n = 1 on a product >= p.
EQUIVALENT_MUTANTS = ("guard_le", "guard_none")


class ModelError(AssertionError):
    """The modelled kernel did something no barrier orders: an unwritten slot read, or a race."""


class Arith:
    """oracle.fe_mul / oracle.fe_add on 32-byte rows, by address; products of a given (a, b) pair
    are computed once per pair (the cases of a sweep are prefixes of one pair), and so are whole
    blocks of the grid kernels (grid_kernel_block: a block is a function of its arguments alone)."""

    def __init__(self, oracle):
        proto = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)
        self.mul = proto((oracle.prefix + "fe_mul", oracle.lib))
        self.add = proto((oracle.prefix + "fe_add", oracle.lib))
        self._pairs = {}
        self.blocks = {}

    def products(self, a, b):
        """Address of the (len(a), 4) array of fe_mul(a[i], b[i]), computed on the pair's first use."""
        key = (id(a), id(b))
        ent = self._pairs.get(key)
        if ent is None:
            assert a.dtype == np.uint64 and b.dtype == np.uint64 and a.flags.c_contiguous and b.flags.c_contiguous
            prod = np.zeros((len(a), 4), np.uint64)
            pa, pb, pp, mul = a.ctypes.data, b.ctypes.data, prod.ctypes.data, self.mul
            for off in range(0, 32 * len(a), 32):
                mul(pp + off, pa + off, pb + off)
            ent = self._pairs[key] = (a, b, prod, pp)   # (a and b are held: their ids stay theirs)
        return ent[3]


class _Lds:
    """A __shared__ fe25519 array: values (when there is arithmetic) and, per slot, the set of
    tokens summed into it, as a bit mask (None: never written)."""

    def __init__(self, slots, arith):
        self.ar = arith
        self.v = np.zeros((slots, 4), np.uint64) if arith else None
        self.base = self.v.ctypes.data if arith else 0
        self.live = [None] * slots

    def addr(self, t):
        return self.base + 32 * t

    def zero(self, t):                       # device_fe25519_0
        if self.ar and self.live[t] is not None:   # (a fresh array is zero already)
            self.v[t] = 0
        self.live[t] = 0

    def store(self, t, src_addr, live):      # device_fe25519_copy / the product written in place
        if self.ar:
            ctypes.memmove(self.addr(t), src_addr, 32)
        self.live[t] = live

    def add_phase(self, pairs):
        """One barrier-to-barrier step: each (tid, src) does s[tid] = s[tid] + s[src]."""
        live, base, slots = self.live, self.base, len(self.live)
        written = read = 0
        for t, src in pairs:
            if src >= slots or live[src] is None or live[t] is None:
                raise ModelError(f"thread {t} reads slot {src}, which no thread wrote")
            written |= 1 << t
            read |= 1 << src
        if bin(written).count("1") != len(pairs):
            raise ModelError("two threads write one slot")
        if written & read:
            raise ModelError(f"slots {_bits(written & read)} are read and written in the same phase")
        add = self.ar.add if self.ar else None
        for t, src in pairs:
            if add:
                add(base + 32 * t, base + 32 * t, base + 32 * src)
            live[t] |= live[src]

    def value(self, t):
        return self.v[t].copy() if self.ar else None


def _bits(mask):
    return [i for i in range(mask.bit_length()) if mask >> i & 1]


def _guard(i, n, mutant):
    if mutant == "guard_le":
        return i <= n
    if mutant == "guard_none":
        return True
    return i < n


def _pow2ceil(x):
    p = 1
    while p < x:
        p <<= 1
    return p


# ---------------------------------------------------------------- :154-183
def shared_kernel(arith, a, b, n, block_dim, mutant=None):
    """field_vector_inner_product_shared_kernel<<<1, block_dim>>> -> (value, bit mask of indices)."""
    s = _Lds(MAX_SHARED_ELEMENTS, arith)
    for tid in range(block_dim):                                   # :163-167
        if tid < n:
            s.store(tid, arith.products(a, b) + 32 * tid if arith else 0, 1 << tid)
        else:
            s.zero(tid)
    stride = block_dim // 2                                        # :171
    if mutant == "tree_ceil":
        stride = (block_dim + 1) // 2
    elif mutant == "tree_pow2":
        stride = _pow2ceil(block_dim) // 2
    while stride > 0:
        s.add_phase([(tid, tid + stride) for tid in range(block_dim)
                     if tid < stride and _guard(tid + stride, n, mutant)])   # :172-174
        stride >>= 1
    return s.value(0), s.live[0]                                   # :179-181


# ---------------------------------------------------------------- :185-216
def ip_shared(arith, a, b, n=None, mutant=None):
    """cuda_field_vector_inner_product_shared -> (value, live indices)."""
    n = len(a) if n is None else n
    num_threads = min(n, MAX_SHARED_ELEMENTS)                      # :204
    v, live = shared_kernel(arith, a, b, n, num_threads, mutant)
    return v, np.array(_bits(live), np.int64)


# ---------------------------------------------------------------- :219-257
def warp_reduce(s, block_dim):
    """warp_reduce_field_element as called at :296-298 (threads tid < WARP_SIZE of the block)."""
    for k in (16, 8, 4, 2, 1):                                     # :223, :229, :235, :241, :247
        s.add_phase([(tid & (WARP_SIZE - 1), (tid & (WARP_SIZE - 1)) + k)
                     for tid in range(min(WARP_SIZE, block_dim)) if (tid & (WARP_SIZE - 1)) < k])


# ---------------------------------------------------------------- :33-61 and :260-299
def grid_kernel_block(arith, a, b, n, block_idx, grid_dim, warp_tail, mutant=None, base=0):
    """Block block_idx of field_vector_inner_product_kernel<<<grid_dim, 256>>> (warp_tail False) or
    of batch_inner_product_kernel's vector at element offset `base` (warp_tail True) ->
    (value block_idx writes, tuple of the index ranges that reach it)."""
    step = grid_dim * BLOCK_SIZE                                   # :50, :283
    if warp_tail and mutant == "batch_stride_block":
        step = BLOCK_SIZE
    one_turn = mutant == "one_turn" and n > step   # (up to n = step no thread takes a second turn)
    key = (id(a), id(b), n, block_idx, step, bool(warp_tail), one_turn, base)
    if arith and key in arith.blocks:
        return arith.blocks[key]
    s = _Lds(BLOCK_SIZE, arith)
    idxs = []
    add, prod = (arith.add, arith.products(a, b) + 32 * base) if arith else (None, 0)
    for tid in range(BLOCK_SIZE):
        s.zero(tid)                                                # :43, :276
        r = range(block_idx * BLOCK_SIZE + tid, n, step)           # :40, :46, :50
        if one_turn:
            r = r[:1]
        idxs.append(r)
        if len(r):
            s.live[tid] = 1 << tid
            if arith:
                acc = s.addr(tid)
                for idx in r:                                      # :47-49
                    add(acc, acc, prod + 32 * idx)
    stride = BLOCK_SIZE // 2
    while stride >= (WARP_SIZE if warp_tail else 1):               # :55-60, :288-293
        s.add_phase([(tid, tid + stride) for tid in range(BLOCK_SIZE) if tid < stride])
        stride >>= 1
    if warp_tail:
        warp_reduce(s, BLOCK_SIZE)                                 # :296-298
    out = (s.value(0), tuple(idxs[t] for t in _bits(s.live[0])))
    if arith:
        arith.blocks[key] = out
    return out


# ---------------------------------------------------------------- :69-92
def reduce_kernel(arith, partial, n, mutant=None):
    """fe25519_reduce_kernel<<<1, 256>>>(result, partials, n); partial(k) -> (value, ranges) of
    partial k, evaluated only when a thread reads it -> (value, bit mask of partial numbers)."""
    block = BLOCK_SIZE
    if mutant == "reduce_255":
        block = 255
    elif mutant == "reduce_257":
        block = 257
    elif mutant == "reduce_all":
        block = max(n, 1)
    s = _Lds(block, arith)
    for tid in range(block):                                       # :75-79
        if tid < n:
            v = partial(tid)[0]
            s.store(tid, v.ctypes.data if arith else 0, 1 << tid)
        else:
            s.zero(tid)
    lim = min(n, block) if block < BLOCK_SIZE else n               # a 255-slot block has no slot 255
    stride = BLOCK_SIZE // 2 if block <= BLOCK_SIZE else _pow2ceil(block) // 2   # :83
    while stride > 0:
        s.add_phase([(tid, tid + stride) for tid in range(block)
                     if tid < stride and tid + stride < block and _guard(tid + stride, lim, mutant)])   # :84-86
        stride >>= 1
    return s.value(0), s.live[0]


def _num_blocks(n, mutant):
    nb = (n + BLOCK_SIZE - 1) // BLOCK_SIZE                        # :123, :332
    cap = {"cap_1023": 1023, "cap_none": None}.get(mutant, MAX_BLOCKS)
    return nb if cap is None else min(nb, cap)                     # :124, :332


def _expand(ranges):
    ranges = [r for r in ranges if len(r)]
    if not ranges:
        return np.zeros(0, np.int64)
    start = np.array([r.start for r in ranges], np.int64)
    step = np.array([r.step for r in ranges], np.int64)
    cnt = np.array([len(r) for r in ranges], np.int64)
    turn = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return np.sort(np.repeat(start, cnt) + np.repeat(step, cnt) * turn)


# ---------------------------------------------------------------- :97-151
def ip_grid(arith, a, b, n=None, mutant=None):
    """cuda_field_vector_inner_product -> (value, live indices)."""
    n = len(a) if n is None else n
    if n <= MAX_SHARED_ELEMENTS:                                   # :108-111
        return ip_shared(arith, a, b, n, mutant)
    num_blocks = _num_blocks(n, mutant)
    memo = {}

    def partial(k):                                                # :134, d_temp[k]
        if k not in memo:
            memo[k] = grid_kernel_block(arith, a, b, n, k, num_blocks, False, mutant)
        return memo[k]
    v, blocks = reduce_kernel(arith, partial, num_blocks, mutant)  # :139
    return v, _expand([r for k in _bits(blocks) for r in partial(k)[1]])


# ---------------------------------------------------------------- :302-347
def ip_batch(arith, a, b, n, num_vectors, mutant=None):
    """cuda_batch_field_vector_inner_product on the contiguous copies (:309-315: vector v at elements
    v * n .. v * n + n - 1 of a and b) -> (values (num_vectors, 4), live indices within a vector)."""
    grid_x = max(_num_blocks(n, mutant), 0)                        # :332
    out = np.zeros((num_vectors, 4), np.uint64) if arith else None
    live = np.zeros(0, np.int64)
    if grid_x == 0:
        return out, live                                           # an empty grid: nothing is written
    for vec in range(num_vectors):                                 # blockIdx.y, :267
        v, ranges = grid_kernel_block(arith, a, b, n, 0, grid_x, True, mutant, base=vec * n)   # x-block 0
        if arith:
            out[vec] = v
        live = _expand(ranges)
    return out, live


# ---------------------------------------------------------------- the swept shapes and their inputs
# One definition for tests/test_ip_orders_ref.py (model == oracle, every mutant told apart) and
# tests/test_ref_surface_shapes_gpu.py (GPU == oracle).
TURN = MAX_BLOCKS * BLOCK_SIZE   # 262144: above it the capped grid's threads take a second turn
SHARED_TAIL_N = (767, 768, 769, 1023, 1024, 1025)
SHARED_ENTRY_N = tuple(range(1, 601)) + SHARED_TAIL_N            # model == oracle.ip_gpu_shared
SHARED_GPU_N = SHARED_ENTRY_N + (5000,)                          # cuda_field_vector_inner_product_shared
DISPATCH_N = tuple(range(1, MAX_SHARED_ELEMENTS + 1))            # cuda_field_vector_inner_product, shared form
GRID_N = tuple(sorted(set(
    [BLOCK_SIZE * nb - r for nb in range(3, 71) for r in (0, 1, 255)] +
    [BLOCK_SIZE * nb - r for nb in (255, 256, 257, 1023, 1024) for r in (0, 37)] +   # full, ragged last block
    [TURN, TURN + 1, TURN + 255, TURN + 256, TURN + 257, 2 * TURN, 2 * TURN + 1, 3 * TURN + 77])))
BATCH_SMALL_N = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000)
BATCH_CASES = tuple((n, nv) for n in BATCH_SMALL_N for nv in (1, 5, 300)) + \
    tuple((n, 2) for n in (TURN, TURN + 1, TURN + 259))
MAX_N = max(GRID_N)

P25519 = 2**255 - 19
MUL_BOUNDED_WORD = 0xFFFFFFEF    # csrc/mul512_asm.h: the product gate's bound on 32-bit words 0 and 7


def fe_int(x):
    return np.array([(x >> (64 * i)) & (2**64 - 1) for i in range(4)], np.uint64)


def edge_pool():
    """(k, 4) uint64: the values a stretch of 64 elements gets one of."""
    M = 2**64 - 1
    r = 0x6A09E667F3BCC908_BB67AE8584CAA73B_3C6EF372FE94F82B_A54FF53A5F1D36F1   # some fixed full-width bits
    vals = [0, 1, P25519 - 1, P25519, P25519 + 1, 2 * P25519, 2**255, 2**256 - 1,
            (r & ~0xFFFFFFFF) | (MUL_BOUNDED_WORD + 1),            # word 0 just above the gate
            (r & ~0xFFFFFFFF) | 0xFFFFFFFF,                        # word 0 all ones
            (r & (2**224 - 1)) | ((MUL_BOUNDED_WORD + 1) << 224),  # word 7 just above the gate
            (r & (2**224 - 1) & ~0xFFFFFFFF) | (0xFFFFFFFF << 224) | 0xFFFFFFFF,   # both
            (r & ~0xFFFFFFFF) | MUL_BOUNDED_WORD]                  # word 0 at the bound: the gate stays shut
    vals += [M << (64 * i) for i in range(4)]                      # one limb of 2^64 - 1
    vals += [(r & ~(M << (64 * i))) | (M << (64 * i)) for i in range(4)]   # ... among random limbs
    vals += [(2**256 - 1) & ~(M << (64 * i)) for i in range(4)]    # three limbs of 2^64 - 1
    return np.stack([fe_int(v) for v in vals])


def draw_inputs(n, seed=20250):
    """Full 256-bit random (a, b), every 64-element stretch of each carrying one pool element; in
    every third stretch the two sit at the same index, so that pool values also meet each other."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    b = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    pool = edge_pool()
    k = np.arange((n + 63) // 64)
    ia = 64 * k + (5 * k) % 64
    ib = 64 * k + (5 * k + np.where(k % 3 == 0, 0, 17)) % 64
    a[ia[ia < n]] = pool[k[ia < n] % len(pool)]
    b[ib[ib < n]] = pool[(k[ib < n] // 3 + 7 * k[ib < n]) % len(pool)]
    return a, b
