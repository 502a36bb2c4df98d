// bp_api_blob.hip — compact proof blobs (bp_codec.h, bp_codec.hip), proof ids and the
// batch Merkle root (bp_ids.h, bp_ids.hip) in the C ABI (include/cudabulletproof_hip.h):
//   hipbp_proof_blob_bound / _header / _parse
//   hipbp_batch_proof_encode / _decode (device), hipbp_proofs_encode_host / _decode_host
//   hipbp_batch_proof_ids, hipbp_blob_proof_ids, hipbp_merkle_root (device)
//   hipbp_proof_ids_host, hipbp_blob_proof_ids_host, hipbp_merkle_root_host / _path_host / _verify_host
// The device and the host forms call the same bodies of bp_codec.h and bp_ids.h.
#include <atomic>
#include <thread>

#include "bp_engine.h"
#include "bp_ids.h"

using namespace bpe;

// What the encoder and the id kernel check of a flat batch, in this order, as entry point `me`.
static int flat_batch_check(const char* me, const hipbp_proof_batch* b, int with_blinding) {
    if (const char* e = bp::codec_shape_error(b->count, b->n, b->ab_len, b->L_len, 0)) return codec_fail(me, e);
    if (b->count && !((b->Vp || b->V) && b->A && b->S && b->T1 && b->T2 && b->t && b->a && b->b && b->c && b->x &&
                      (!b->L_len || (b->L && b->R))))
        return codec_fail(me, "null batch field");
    if (with_blinding && b->count && (!b->taux || !b->mu)) return codec_fail(me, "with_blinding needs the batch's taux and mu");
    return HIPBP_OK;
}
// ... of a blob's info (*l: its layout) ...
static int blob_info_check(const char* me, const hipbp_proof_blob_info* info, bp::CodecLayout* l) {
    if (const char* e = bp::codec_shape_error(info->count, info->n, info->ab_len, info->L_len, info->flags))
        return codec_fail(me, e);
    *l = bp::codec_layout(*info);
    if (info->raw_count > info->count || l->bytes(info->raw_count) != info->bytes || (l->Sc() == 0 && info->raw_count != info->count))
        return codec_fail(me, "info does not describe a blob (use hipbp_proof_blob_header)");
    return HIPBP_OK;
}
// ... and of host structs: one shape, the first proof's (*abl, *Lr)
static int host_proofs_check(const char* me, const RangeProof* proofs, size_t count, size_t n, size_t* abl, size_t* Lr) {
    *abl = count ? proofs[0].ip_proof.a.length : 1;
    *Lr = count ? proofs[0].ip_proof.L_len : 0;
    for (size_t i = 0; i < count; i++) {
        const InnerProductProof& ip = proofs[i].ip_proof;
        if (ip.a.length != *abl || ip.b.length != *abl || ip.L_len != *Lr || ip.L.length < *Lr || ip.R.length < *Lr ||
            !ip.a.elements || !ip.b.elements || (*Lr && (!ip.L.elements || !ip.R.elements)))
            return codec_fail(me, ("proof " + std::to_string(i) +
                                   ": another shape than the first proof's, or inconsistent vector lengths").c_str());
    }
    if (const char* e = bp::codec_shape_error(count, n, *abl, *Lr, 0)) return codec_fail(me, e);
    return HIPBP_OK;
}

// the arrays of one host struct as a one-proof batch (index 0): nothing is copied
static bp::CodecArrays arrays_of_struct(const RangeProof& p) {
    RangeProof& q = const_cast<RangeProof&>(p);   // (the encoder only reads)
    bp::CodecArrays A;
    ge25519* pts[5] = {&q.V, &q.A, &q.S, &q.T1, &q.T2};
    for (int k = 0; k < 5; k++) A.pt[k] = (bp::ge*)pts[k];
    A.t = (bp::fe*)&q.t; A.c = (bp::fe*)&q.ip_proof.c; A.x = (bp::fe*)&q.ip_proof.x;
    A.taux = (bp::fe*)&q.taux; A.mu = (bp::fe*)&q.mu;
    A.a = (bp::fe*)q.ip_proof.a.elements; A.b = (bp::fe*)q.ip_proof.b.elements;
    A.L = (bp::ge*)q.ip_proof.L.elements; A.R = (bp::ge*)q.ip_proof.R.elements;
    return A;
}
static void free_proof_vectors(RangeProof& p) {
    free(p.ip_proof.a.elements); free(p.ip_proof.b.elements);
    free(p.ip_proof.L.elements); free(p.ip_proof.R.elements);
}

// the stream's ids workspace grown for a root over `leaves` ids / a blob of `count` proofs
static int ids_workspace(Engine* e, hipStream_t s, size_t leaves, size_t count, bp::IdsWs& w) {
    Buf(&ib)[bp::IDB_COUNT] = e->streams[s].ids;
    size_t sz[bp::IDB_COUNT];
    bp::ids_sizes(leaves, count, sz);
    // (a grown buffer frees the old one: the stream's earlier call may still use it)
    bool grow = false;
    for (int k = 0; k < bp::IDB_COUNT; k++) grow = grow || (sz[k] > ib[k].cap && ib[k].p);
    if (grow) BP_RET_ON(hipStreamSynchronize(s));
    BP_RET_ON(need_all(ib, sz));
    {
        using namespace bp;
        Buf(&b)[IDB_COUNT] = ib;
        BP_IDS_BUFS(BP_BUF_FIELD)
    }
    return HIPBP_OK;
}

// fn(lo, hi) over [0, count) in contiguous parts on HIPBP_HOST_THREADS threads (unset: the machine's,
// 16 at most; at least 256 items a thread, so a small batch stays on the caller's thread)
template <class F>
static void host_parts(size_t count, F fn) {
    const char* env = getenv("HIPBP_HOST_THREADS");
    size_t nt = env && atoi(env) > 0 ? (size_t)atoi(env) : std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));
    nt = std::min(nt, (count + 255) / 256);
    if (nt <= 1) {
        fn((size_t)0, count);
        return;
    }
    std::vector<std::thread> workers;
    for (size_t k = 0; k < nt; k++) workers.emplace_back(fn, count * k / nt, count * (k + 1) / nt);
    for (auto& w : workers) w.join();
}

extern "C" {

size_t hipbp_proof_blob_bound(size_t count, size_t ab_len, size_t L_len, unsigned flags) {
    return bp::CodecLayout{count, ab_len, L_len, (int)(flags & 1)}.bound();
}

int hipbp_proof_blob_header(const uint8_t* header32, size_t blob_bytes, hipbp_proof_blob_info* info) {
    if (!header32 || !info) return codec_fail("proof_blob_header", "null argument");
    if (const char* e = bp::codec_parse_header(header32, blob_bytes, info)) return codec_fail("proof_blob_header", e);
    return HIPBP_OK;
}

int hipbp_proof_blob_parse(const uint8_t* blob, size_t bytes, hipbp_proof_blob_info* info) {
    if (!info) return codec_fail("proof_blob_parse", "null argument");
    if (const char* e = bp::codec_parse(blob, bytes, info)) return codec_fail("proof_blob_parse", e);
    return HIPBP_OK;
}

int hipbp_batch_proof_encode(const hipbp_proof_batch* b, int with_blinding, uint8_t* blob_dev, size_t cap,
                             uint64_t* bytes_out_dev, void* stream) {
    if (!b || !blob_dev || !bytes_out_dev) return codec_fail("proof_encode", "null argument");
    if (int rc = flat_batch_check("proof_encode", b, with_blinding)) return rc;
    if ((uintptr_t)blob_dev % 8) return codec_fail("proof_encode", "blob_dev must be 8-byte aligned");
    const bp::CodecLayout l{b->count, b->ab_len, b->L_len, with_blinding ? 1 : 0};
    if (cap < l.bound()) return codec_fail("proof_encode", "cap below hipbp_proof_blob_bound");
    BP_ENGINE_OR_RET(e);
    const bp::CodecArrays A = bp::codec_arrays(*b, true, with_blinding != 0);
    std::lock_guard<std::mutex> lk(e->mu);
    Buf(&cb)[bp::CDB_COUNT] = e->streams[pick(stream)].codec;
    size_t sz[bp::CDB_COUNT];
    bp::codec_sizes(b->count, sz);
    // (a grown buffer frees the old one: the stream's earlier encode may still read it)
    if (sz[bp::CDB_BLK] > cb[bp::CDB_BLK].cap && cb[bp::CDB_BLK].p) BP_RET_ON(hipStreamSynchronize(pick(stream)));
    BP_RET_ON(need_all(cb, sz));
    bp::CodecWs w;
    {
        using namespace bp;
        Buf(&b)[CDB_COUNT] = cb;
        BP_CODEC_BUFS(BP_BUF_FIELD)
    }
    bp::launch_codec_encode(A, l, b->n, blob_dev, w, bytes_out_dev, pick(stream));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_batch_proof_decode(const uint8_t* blob_dev, const hipbp_proof_blob_info* info, hipbp_proof_out* o,
                             uint32_t* bad_dev, void* stream) {
    if (!blob_dev || !info || !o || !bad_dev) return codec_fail("proof_decode", "null argument");
    bp::CodecLayout l;
    if (int rc = blob_info_check("proof_decode", info, &l)) return rc;
    if ((uintptr_t)blob_dev % 8) return codec_fail("proof_decode", "blob_dev must be 8-byte aligned");
    if (info->count && !(o->V && o->A && o->S && o->T1 && o->T2 && o->t && o->c && o->x && o->a && o->b &&
                         (!l.Lr || (o->L && o->R)) && (!l.f || (o->taux && o->mu))))
        return codec_fail("proof_decode", "null output array");
    BP_ENGINE_OR_RET(e);
    (void)e;
    const bp::CodecArrays A = bp::codec_arrays(*o, l.f != 0);
    BP_RET_ON(hipMemsetAsync(bad_dev, 0, sizeof(uint32_t), pick(stream)));
    bp::launch_codec_decode(bp::codec_view(blob_dev, info->bytes, l, info->raw_count), A, l, bad_dev, pick(stream));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_proofs_encode_host(const RangeProof* proofs, size_t count, size_t n, int with_blinding, uint8_t* blob,
                             size_t cap, size_t* bytes) {
    if (!blob || !bytes || (count && !proofs)) return codec_fail("proofs_encode_host", "null argument");
    size_t abl, Lr;
    if (int rc = host_proofs_check("proofs_encode_host", proofs, count, n, &abl, &Lr)) return rc;
    const bp::CodecLayout l{count, abl, Lr, with_blinding ? 1 : 0};
    if (cap < l.bound()) return codec_fail("proofs_encode_host", "cap below hipbp_proof_blob_bound");
    // the device encoder's three steps, one proof at a time through the same bodies
    uint8_t* kind = blob + l.o_kind();
    memset(kind, 0, bp::pad8(count));
    size_t R = 0;
    for (size_t i = 0; i < count; i++) R += kind[i] = bp::codec_classify(arrays_of_struct(proofs[i]), l, 0);
    uint8_t* ridx = blob + l.o_rawidx();
    memset(ridx, 0, bp::pad8(4 * R));
    size_t j = 0;
    for (size_t i = 0; i < count; i++) {
        const bp::CodecArrays A = arrays_of_struct(proofs[i]);
        bp::codec_write_compact(blob + l.o_compact() + i * l.Sc(), A, l, 0, kind[i]);
        if (!kind[i]) continue;
        bp::put_le(ridx + 4 * j, i, 4);
        bp::codec_write_raw(blob + l.o_raw(R) + j * l.Sr(), A, l, 0);
        j++;
    }
    bp::codec_write_header(blob, l, n, R);
    *bytes = l.bytes(R);
    return HIPBP_OK;
}

int hipbp_proofs_decode_host(const uint8_t* blob, size_t bytes, RangeProof* proofs) {
    hipbp_proof_blob_info info;
    if (const char* e = bp::codec_parse(blob, bytes, &info)) return codec_fail("proofs_decode_host", e);
    if (info.count == 0) return HIPBP_OK;
    if (!proofs) return codec_fail("proofs_decode_host", "null proofs");
    const bp::CodecLayout l = bp::codec_layout(info);
    const size_t R = info.raw_count;
    memset(proofs, 0, info.count * sizeof(RangeProof));
    size_t j = 0, bad = 0, i = 0;
    bool oom = false;
    for (; i < info.count && !bad && !oom; i++) {
        RangeProof& p = proofs[i];
        if (!bp::proof_vectors_alloc(p.ip_proof, info.n, l.Lr, malloc, l.abl)) { oom = true; i++; break; }
        const uint8_t k = blob[l.o_kind() + i];
        bp::BlobView v;
        v.kind = blob + l.o_kind() + i; v.compact = blob + l.o_compact() + i * l.Sc();
        v.rawidx = blob + l.o_rawidx() + 4 * j; v.raw = blob + l.o_raw(R) + j * l.Sr();
        v.count = 1; v.R = k; v.base = i;
        v.kind_n = v.compact_n = 1; v.rawidx_n = v.raw_n = k;
        bp::CodecArrays A = arrays_of_struct(p);
        if (!l.f) A.taux = A.mu = nullptr;
        bad += bp::codec_decode_cpu(v, A, l);
        j += k;
    }
    if (bad || oom) {   // nothing stays allocated, every struct zero
        for (size_t k = 0; k < i; k++) free_proof_vectors(proofs[k]);
        memset(proofs, 0, info.count * sizeof(RangeProof));
        if (oom) { g_err = "proofs_decode_host: out of memory"; return HIPBP_ERR_DEVICE; }
        return codec_fail("proofs_decode_host", "a record failed its checks");
    }
    return HIPBP_OK;
}

int hipbp_batch_proof_ids(const hipbp_proof_batch* b, int with_blinding, uint8_t* ids_dev, uint8_t* kind_dev,
                          void* stream) {
    if (!b || (b->count && !ids_dev)) return codec_fail("proof_ids", "null argument");
    if (int rc = flat_batch_check("proof_ids", b, with_blinding)) return rc;
    if ((uintptr_t)ids_dev % 4) return codec_fail("proof_ids", "ids_dev must be 4-byte aligned");
    if (b->count == 0) return HIPBP_OK;
    const bp::CodecLayout l{b->count, b->ab_len, b->L_len, with_blinding ? 1 : 0};
    BP_ENGINE_OR_RET(e);
    (void)e;
    bp::launch_proof_ids(bp::codec_arrays(*b, true, with_blinding != 0), l, b->n, ids_dev, kind_dev, pick(stream));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_blob_proof_ids(const uint8_t* blob_dev, const hipbp_proof_blob_info* info, uint8_t* ids_dev, uint32_t* bad_dev,
                         void* stream) {
    if (!blob_dev || !info || !bad_dev || (info->count && !ids_dev)) return codec_fail("blob_proof_ids", "null argument");
    bp::CodecLayout l;
    if (int rc = blob_info_check("blob_proof_ids", info, &l)) return rc;
    if ((uintptr_t)blob_dev % 8) return codec_fail("blob_proof_ids", "blob_dev must be 8-byte aligned");
    if ((uintptr_t)ids_dev % 4 || (uintptr_t)bad_dev % 4) return codec_fail("blob_proof_ids", "ids_dev and bad_dev must be 4-byte aligned");
    BP_ENGINE_OR_RET(e);
    std::lock_guard<std::mutex> lk(e->mu);
    bp::IdsWs w;
    if (int rc = ids_workspace(e, pick(stream), 0, info->count, w)) return rc;
    bp::launch_blob_ids(bp::codec_view(blob_dev, info->bytes, l, info->raw_count), l, info->n, ids_dev, w, bad_dev, pick(stream));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_merkle_root(const uint8_t* ids_dev, size_t count, uint8_t* root_dev, void* stream) {
    if (!root_dev || (count && !ids_dev)) return codec_fail("merkle_root", "null argument");
    if (count > bp::MERKLE_MAX_COUNT) return codec_fail("merkle_root", "count above 2^24");
    if ((uintptr_t)ids_dev % 4 || (uintptr_t)root_dev % 4) return codec_fail("merkle_root", "ids_dev and root_dev must be 4-byte aligned");
    BP_ENGINE_OR_RET(e);
    std::lock_guard<std::mutex> lk(e->mu);
    bp::IdsWs w;
    if (int rc = ids_workspace(e, pick(stream), count, 0, w)) return rc;
    bp::launch_merkle_root(ids_dev, count, root_dev, w, pick(stream));
    BP_RET_ON(hipGetLastError());
    return HIPBP_OK;
}

int hipbp_proof_ids_host(const RangeProof* proofs, size_t count, size_t n, int with_blinding, uint8_t* ids) {
    if (count && (!proofs || !ids)) return codec_fail("proof_ids_host", "null argument");
    size_t abl, Lr;
    if (int rc = host_proofs_check("proof_ids_host", proofs, count, n, &abl, &Lr)) return rc;
    const bp::CodecLayout l{count, abl, Lr, with_blinding ? 1 : 0};
    host_parts(count, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) bp::ids_flat_proof(arrays_of_struct(proofs[i]), l, n, 0, ids + bp::ID_BYTES * i);
    });
    return HIPBP_OK;
}

int hipbp_blob_proof_ids_host(const uint8_t* blob, size_t bytes, uint8_t* ids) {
    hipbp_proof_blob_info info;
    if (const char* e = bp::codec_parse(blob, bytes, &info)) return codec_fail("blob_proof_ids_host", e);
    if (info.count && !ids) return codec_fail("blob_proof_ids_host", "null ids");
    const bp::CodecLayout l = bp::codec_layout(info);
    const bp::BlobView v = bp::codec_view(blob, bytes, l, info.raw_count);
    std::atomic<size_t> bad{0};
    host_parts(info.count, [&](size_t lo, size_t hi) {
        size_t b = 0;
        for (size_t i = lo; i < hi; i++) b += bp::ids_blob_proof(v, l, info.n, i, ids + bp::ID_BYTES * i);
        bad += b;
    });
    if (bad) {   // (not after a full parse)
        memset(ids, 0, info.count * bp::ID_BYTES);
        return codec_fail("blob_proof_ids_host", "a record failed its checks");
    }
    return HIPBP_OK;
}

int hipbp_merkle_root_host(const uint8_t* ids, size_t count, uint8_t root[32]) {
    if (!root || (count && !ids)) return codec_fail("merkle_root_host", "null argument");
    if (count > bp::MERKLE_MAX_COUNT) return codec_fail("merkle_root_host", "count above 2^24");
    if (count == 0) {
        uint32_t d[8];
        bp::merkle_empty(d);
        bp::ids_store(root, d);
        return HIPBP_OK;
    }
    std::vector<std::vector<uint8_t>> lv;
    bp::merkle_levels_cpu(ids, count, lv);
    memcpy(root, lv.back().data(), bp::ID_BYTES);
    return HIPBP_OK;
}

int hipbp_merkle_path_host(const uint8_t* ids, size_t count, size_t index, uint8_t* path, size_t* path_len) {
    if (!ids || !path || !path_len) return codec_fail("merkle_path_host", "null argument");
    if (count > bp::CODEC_MAX_COUNT) return codec_fail("merkle_path_host", "count above 2^22");
    if (index >= count) return codec_fail("merkle_path_host", "index not below count");
    std::vector<std::vector<uint8_t>> lv;
    bp::merkle_levels_cpu(ids, count, lv);
    *path_len = bp::merkle_path_cpu(lv, count, index, path);
    return HIPBP_OK;
}

int hipbp_merkle_verify_host(const uint8_t id[32], size_t index, size_t count, const uint8_t* path, size_t path_len,
                             const uint8_t root[32]) {
    if (!id || !root || (path_len && !path)) return 0;
    return bp::merkle_verify_cpu(id, index, count, path, path_len, root) ? 1 : 0;
}

}  // extern "C"
