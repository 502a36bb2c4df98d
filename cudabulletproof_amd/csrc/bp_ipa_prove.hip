// bp_ipa_prove.hip — gfx950 kernels for the reference's stand-alone inner_product_prove
// (bulletproof_vectors.cu:277-523) at any power-of-two n, bit-exact, batched.
//
// bp_prove.hip runs the range proof's IPA rounds one lane per proof over all O(n) products, folds
// and work-list entries: fine at n = 64 with 65,536 proofs, a serial loop at n = 4096 with a handful.
// Here every O(n) piece of a round is one lane per element or per term over all proofs of a chunk;
// a per-proof (per-chain) lane only ever loops over additions whose ORDER the reference fixes (this
// arithmetic is not associative).  Round r of a chunk, n' = n >> (r + 1):
//   k_ipa_elem     lane/term    the 4n' canonical MSM scalars a_L | b_R | a_R | b_L, the 2n' products
//                               a_L_j b_R_j, a_R_j b_L_j, the heavy scalars' chain-length histogram
//   k_ipa_cchain   lane/chain   c_L, c_R: the two sequential fe_add chains over the products
//   (scan)                      histogram -> start offsets, longest chains first
//   k_ipa_scatter  lane/item    zero scalars: the constant term; heavy items into the chain-length
//                               order, light ones (<= 64 bits) behind them; block-level reservation
//   k_ipa_terms    lane/item    the scalar multiplications (4n' MSM terms, c_L Q, c_R Q), grid-stride
//   k_ipa_pchain   lane/chain   the four sequential point chains of point_vector_multi_scalar_mul
//   k_ipa_round    lane/proof   L, R, the challenge u, u^-1, the transcript
//   k_ipa_fold     lane/element a' = u^-1 a_L + u a_R, b' = u b_L + u^-1 b_R
// The field chains are done before the term launch, so c_L Q and c_R Q ride in the same launch as
// the MSM terms and the point chains wait for nothing but their own terms.
#include "bp_kernels.h"
#include "ge25519_dev.h"
#include "sha256_dev.h"

namespace bp {

namespace {
constexpr int TPB = 256;
__device__ __forceinline__ size_t gid() { return (size_t)blockIdx.x * blockDim.x + threadIdx.x; }
inline unsigned nblk(size_t items) { return (unsigned)((items + TPB - 1) / TPB); }

// 0 zero (a constant term), 1 light (<= 64 significant bits), 2 heavy
__device__ __forceinline__ int sclass(const fe& s) {
    if (s.v[3] | s.v[2] | s.v[1]) return 2;
    return s.v[0] ? 1 : 0;
}

// IpaWs::ctl: [0, MSM_BINS) the heavy items' chain-length bins (then their start offsets),
// [MSM_BINS] the heavy count, [MSM_BINS + 1] the light count
constexpr int CTL_HEAVY = MSM_BINS, CTL_LIGHT = MSM_BINS + 1;

// Block-level histogram of the heavy scalars' chain lengths: LDS counts, then one global atomic per
// (block, non-empty bin) and one for the block's heavy count.  Every lane of the block calls it.
__device__ __forceinline__ void block_hist(const IpaWs& ws, unsigned* hb, bool heavy, int key) {
    for (int k = threadIdx.x; k <= MSM_BINS; k += TPB) hb[k] = 0;
    __syncthreads();
    if (heavy) {
        atomicAdd(&hb[key], 1u);
        atomicAdd(&hb[MSM_BINS], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k <= MSM_BINS; k += TPB)
        if (hb[k]) atomicAdd(&ws.ctl[k], hb[k]);
}
}  // namespace

// ---------------------------------------------------------------- per-term scalars and products
// lane (p, k), k < 4n': blocks a_L | b_R | a_R | b_L of n' scalars each (vectors.cu:365-370, :397-398,
// :431-432), in tobytes form; the a-side lanes also form the round's product a_L_j b_R_j (block 0) or
// a_R_j b_L_j (block 2) for the c_L / c_R chains (products in any order, the additions not).
__global__ __launch_bounds__(TPB) void k_ipa_elem(IpaWs ws, int np) {
    __shared__ unsigned hb[MSM_BINS + 1];
    const size_t i = gid(), per = 4 * (size_t)np;
    const bool live = i < (size_t)ws.B * per;
    bool heavy = false;
    int key = 0;
    if (live) {
        const size_t p = i / per;
        const int k = (int)(i % per), blk = k / np, j = k % np;
        const size_t n = (size_t)ws.n;
        const fe* a = ws.a + p * n;
        const fe* b = ws.b + p * n;
        const int hi = (blk == 1 || blk == 2) ? np : 0;     // block 0: a_L, 1: b_R, 2: a_R, 3: b_L
        const fe src = (blk & 1) ? b[hi + j] : a[hi + j];
        const fe s = fe_canon(src);
        ws.sc[p * 2 * n + k] = s;
        if (!(blk & 1))                                     // block 0: a_L_j b_R_j, block 2: a_R_j b_L_j
            ws.prod[p * n + hi + j] = fe_mul(src, b[(np - hi) + j]);
        heavy = sclass(s) == 2;
        if (heavy) key = sm_ops_prefix(s, ws.ptab ? ws.pbits : 0);
    }
    block_hist(ws, hb, heavy, key);
}

// ---------------------------------------------------------------- c_L, c_R
// field_vector_inner_product (vectors.cu:101-114): acc = add(acc, mul(a_j, b_j)) from 0 in index
// order; the products are k_ipa_elem's.  Lane (p, side): side 0 c_L = <a_L, b_R>, 1 c_R = <a_R, b_L>.
__global__ __launch_bounds__(TPB) void k_ipa_cchain(IpaWs ws, int np) {
    __shared__ unsigned hb[MSM_BINS + 1];
    const size_t c = gid();
    const bool live = c < (size_t)ws.B * 2;
    bool heavy = false;
    int key = 0;
    if (live) {
        const fe* pr = ws.prod + (c >> 1) * (size_t)ws.n + (c & 1) * (size_t)np;
        fe acc = fe_set(0);
        for (int j = 0; j < np; j++) acc = fe_add(acc, pr[j]);
        const fe s = fe_canon(acc);
        ws.csc[c] = s;
        heavy = sclass(s) == 2;
        if (heavy) key = sm_ops_prefix(s, ws.ptab ? ws.pbits : 0);
    }
    block_hist(ws, hb, heavy, key);
}

// item k of proof p (4n' + 2 items per proof): the MSM scalars, then c_L, c_R
__device__ __forceinline__ fe item_scalar(const IpaWs& ws, size_t p, int k, int np) {
    return k < 4 * np ? ws.sc[p * 2 * (size_t)ws.n + k] : ws.csc[p * 2 + (k - 4 * np)];
}
__device__ __forceinline__ ge* item_term(const IpaWs& ws, size_t p, int k, int np) {
    return k < 4 * np ? ws.term + p * 2 * (size_t)ws.n + k : ws.cq + p * 2 + (k - 4 * np);
}

// ---------------------------------------------------------------- work lists
// A zero scalar's term is a constant (ge25519_scalarmult doubles the identity 256 times whatever the
// point: dtab[256], host-normalized dtab[257]; c Q is not normalized) and is written here.  The heavy
// items go to slist in chain-length order (ws.ctl's bins hold the start offsets by now), the light
// ones to llist; a block reserves its ranges with one global atomic per non-empty bin.
__global__ __launch_bounds__(TPB) void k_ipa_scatter(IpaWs ws, int np, const ge* __restrict__ dtab) {
    __shared__ unsigned cnt[MSM_BINS + 1], base[MSM_BINS + 1];
    for (int k = threadIdx.x; k <= MSM_BINS; k += TPB) cnt[k] = 0;
    __syncthreads();
    const size_t i = gid(), per = 4 * (size_t)np + 2;
    int key = -1;
    unsigned rank = 0;
    if (i < (size_t)ws.B * per) {
        const size_t p = i / per;
        const int k = (int)(i % per);
        const fe s = item_scalar(ws, p, k, np);
        const int c = sclass(s);
        if (c == 0) *item_term(ws, p, k, np) = dtab[k < 4 * np ? 257 : 256];
        else key = c == 2 ? sm_ops_prefix(s, ws.ptab ? ws.pbits : 0) : MSM_BINS;
        if (key >= 0) rank = atomicAdd(&cnt[key], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k <= MSM_BINS; k += TPB)
        if (cnt[k]) base[k] = atomicAdd(&ws.ctl[k < MSM_BINS ? k : CTL_LIGHT], cnt[k]);
    __syncthreads();
    if (key >= 0) (key < MSM_BINS ? ws.slist : ws.llist)[base[key] + rank] = (uint32_t)i;
}

// ---------------------------------------------------------------- scalar multiplications
// item k of proof p: a_L_j G[n'+j] | b_R_j H[j] | a_R_j G[j] | b_L_j H[n'+j] (host-normalized MSM terms,
// vectors.cu:204-206) | c_L Q | c_R Q (raw, :402-404, :435-437).  G, H are the ORIGINAL generators in
// every round.  Grid-stride over the queued items (heavy in chain-length order, then light), one
// scalar-mult call site (two in one wave would run both loops back to back).  Bounded to 4 waves per SIMD
// (128 VGPRs): with the voted lane step a 3-wave bound lets the allocator take 136 and lose the fourth wave.
__global__ __launch_bounds__(TPB, 4) void k_ipa_terms(IpaWs ws, int np, const ge* __restrict__ G,
                                                   const ge* __restrict__ H, const ge* __restrict__ Q,
                                                   const ge* __restrict__ dtab) {
    __shared__ geq qs[TPB];
    const int n = ws.n;
    const size_t per = 4 * (size_t)np + 2;
    const unsigned ch = ws.ctl[CTL_HEAVY], cl = ws.ctl[CTL_LIGHT];
    for (size_t i = gid(); i < (size_t)ch + cl; i += (size_t)gridDim.x * TPB) {
        const uint32_t id = i < ch ? ws.slist[i] : ws.llist[i - ch];
        const size_t p = id / per;
        const int k = (int)(id % per);
        const bool msm = k < 4 * np;
        ge P;
        int base;   // the base's prefix-table row: G_k at k, H_k at n + k, Q (= the set's h) at 2n
        if (msm) {
            const int blk = k / np, j = k % np;
            P = blk == 0 ? G[np + j] : blk == 1 ? H[j] : blk == 2 ? G[j] : H[np + j];
            base = blk == 0 ? np + j : blk == 1 ? n + j : blk == 2 ? j : n + np + j;
        } else {
            P = *Q;
            base = 2 * n;
        }
        const fe s = item_scalar(ws, p, k, np);
        const ge* pt = ws.ptab ? ws.ptab + ((size_t)base << ws.pbits) : nullptr;
        ge r = scalarmult<true>(s, P, &qs[threadIdx.x], dtab, pt, pt ? ws.pbits : 0);
        *item_term(ws, p, k, np) = msm ? ge_norm_host(r) : r;
    }
}

// ---------------------------------------------------------------- point chains
// point_vector_multi_scalar_mul's accumulation (vectors.cu:208-223): acc = t_0, then acc = N(acc + t_i)
// in index order, one final N.  Lane (p, c): chain c of proof p over its n' terms.
__global__ __launch_bounds__(TPB) void k_ipa_pchain(IpaWs ws, int np) {
    const size_t c = gid();
    if (c >= (size_t)ws.B * 4) return;
    const ge* t = ws.term + (c >> 2) * 2 * (size_t)ws.n + (c & 3) * (size_t)np;
    ge acc = t[0];
    for (int i = 1; i < np; i++) acc = ge_norm_host(ge_add(acc, t[i]));
    ws.chain[c] = ge_norm_host(acc);
}

// ---------------------------------------------------------------- L, R, challenge
__global__ __launch_bounds__(TPB) void k_ipa_round(IpaWs ws, int r) {
    const size_t p = gid();
    if (p >= (size_t)ws.B) return;
    const ge* ch = ws.chain + p * 4;
    const ge* tq = ws.cq + p * 2;
    const ge L = ge_norm_host(ge_add(ge_add(ge_add(ge_zero(), ch[0]), ch[1]), tq[0]));   // vectors.cu:406-409
    const ge R = ge_norm_host(ge_add(ge_add(ge_add(ge_zero(), ch[2]), ch[3]), tq[1]));   // :440-443
    ws.L[p * ws.Lr + r] = L;
    ws.R[p * ws.Lr + r] = R;
    const fe u = chal_ip(ws.tr[p], L.X, R.X);   // vectors.cu:448-469; transcript <- the challenge bytes
    ws.tr[p] = u;
    if (r == 0) ws.x[p] = u;                    // proof->x (:472-474)
    ws.uu[p * 2] = u;
    ws.uu[p * 2 + 1] = fe_invert(u);
}

// ---------------------------------------------------------------- fold (vectors.cu:488-500)
// lane (p, j), j < n': reads a[j], a[n'+j], b[j], b[n'+j] and writes a[j], b[j]: no other lane touches them
__global__ __launch_bounds__(TPB) void k_ipa_fold(IpaWs ws, int np) {
    const size_t i = gid();
    if (i >= (size_t)ws.B * np) return;
    const size_t p = i / np;
    const int j = (int)(i % np);
    const fe u = ws.uu[p * 2], ui = ws.uu[p * 2 + 1];
    fe* a = ws.a + p * (size_t)ws.n;
    fe* b = ws.b + p * (size_t)ws.n;
    const fe na = fe_add(fe_mul(ui, a[j]), fe_mul(u, a[np + j]));
    const fe nb = fe_add(fe_mul(u, b[j]), fe_mul(ui, b[np + j]));
    a[j] = na;
    b[j] = nb;
}

// ---------------------------------------------------------------- inputs / outputs
// a, b <- the caller's vectors (folded in place from here on), the transcript's raw limbs, x = 0
__global__ __launch_bounds__(TPB) void k_ipa_load(IpaWs ws, const fe* __restrict__ a, const fe* __restrict__ b,
                                                  const fe* __restrict__ tr) {
    const size_t i = gid(), m = (size_t)ws.B * ws.n;
    if (i < m) {
        ws.a[i] = a[i];
        ws.b[i] = b[i];
    }
    if (i < (size_t)ws.B) {
        ws.tr[i] = tr ? tr[i] : fe_set(0);
        ws.x[i] = fe_set(0);
    }
}

// the final length-1 a, b; c = c_in as given; x; c_final = field_vector_inner_product of the final a, b
__global__ __launch_bounds__(TPB) void k_ipa_final(IpaWs ws, const fe* __restrict__ c_in, fe* a, fe* b, fe* c,
                                                   fe* x, fe* c_final) {
    const size_t p = gid();
    if (p >= (size_t)ws.B) return;
    const fe fa = ws.a[p * (size_t)ws.n], fb = ws.b[p * (size_t)ws.n];
    a[p] = fa;
    b[p] = fb;
    c[p] = c_in[p];
    x[p] = ws.x[p];
    if (c_final) c_final[p] = fe_add(fe_set(0), fe_mul(fa, fb));
}

void launch_ipa_load(const IpaWs& ws, const fe* a, const fe* b, const fe* tr, hipStream_t s) {
    k_ipa_load<<<nblk((size_t)ws.B * ws.n), TPB, 0, s>>>(ws, a, b, tr);
}

void launch_ipa_round(const IpaWs& ws, int r, const ge* G, const ge* H, const ge* Q, const ge* dtab,
                      hipStream_t s) {
    const int np = ws.n >> (r + 1);
    const size_t B = (size_t)ws.B, items = B * (4 * (size_t)np + 2);
    (void)hipMemsetAsync(ws.ctl, 0, (MSM_BINS + 2) * sizeof(unsigned), s);
    k_ipa_elem<<<nblk(B * 4 * np), TPB, 0, s>>>(ws, np);
    k_ipa_cchain<<<nblk(B * 2), TPB, 0, s>>>(ws, np);
    launch_ops_scan(ws.ctl, 1, s);   // bins -> start offsets, longest chains first
    k_ipa_scatter<<<nblk(items), TPB, 0, s>>>(ws, np, dtab);
    // at most TERMS_BLOCKS blocks (4 waves per SIMD over the GPU), grid-stride over the items
    constexpr unsigned TERMS_BLOCKS = 1024;
    const unsigned nb = nblk(items);
    k_ipa_terms<<<nb < TERMS_BLOCKS ? nb : TERMS_BLOCKS, TPB, 0, s>>>(ws, np, G, H, Q, dtab);
    k_ipa_pchain<<<nblk(B * 4), TPB, 0, s>>>(ws, np);
    k_ipa_round<<<nblk(B), TPB, 0, s>>>(ws, r);
    k_ipa_fold<<<nblk(B * np), TPB, 0, s>>>(ws, np);
}

void launch_ipa_final(const IpaWs& ws, const fe* c_in, fe* a, fe* b, fe* c, fe* x, fe* c_final, hipStream_t s) {
    k_ipa_final<<<nblk((size_t)ws.B), TPB, 0, s>>>(ws, c_in, a, b, c, x, c_final);
}

}  // namespace bp
