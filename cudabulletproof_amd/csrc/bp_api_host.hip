// bp_api_host.hip — the entry points of the C ABI (include/cudabulletproof_hip.h) on host data, each
// synchronous and cut into shards over the devices by HostFan (bp_engine.h):
//   hipbp_batch_generate_range_proof_host / _host_sharded, hipbp_batch_generate_range_proof_accepted_host
//   hipbp_batch_pedersen_commit_host
//   hipbp_batch_range_proof_verify_host, hipbp_batch_range_proof_verify_bytes_host
#include "bp_engine.h"
#include "bp_codec.h"

using namespace bpe;

namespace {

// ---- the provers on host data.  A call is cut into shards (one host thread and one
// device each) and every shard into chunks, by bp_host_prove.h's plan; the shards' results go to
// the caller through its ProofOwner, which also undoes them all if any shard fails.
struct HostProveCall {
    const fe25519 *v, *gamma;
    size_t n;
    const PointVector *G, *H;
    const ge25519 *g, *h;
    const uint8_t* seed32;
    int max_attempts, check;      // the accepted prover's (max_attempts = 0: the seeded prover)
    size_t piece;                 // ... and the proofs per piece of a chunk's way back to the host
    bp::ProofOwner* own;
};

// A shard's hold on its device's prove-host staging: the engine's two streams, the pinned and the
// device buffer grown to hold the packed generators at their offsets (the shard's slots lie in
// front of them), the generators uploaded on stream 0 and stream 1 made to wait for them.  It keeps
// prove_host_mu until it goes out of scope: shards and calls on one device run one after another,
// and each leaves both streams drained of its work, so nothing still reads the staging when it grows.
struct HostStage {
    Engine* e = nullptr;
    std::unique_lock<std::mutex> hold;
    hipStream_t st[2] = {nullptr, nullptr};
    bool streams = false;
    uint8_t *host = nullptr, *dbuf = nullptr;
    GenView gens;   // the device copy
    hipEvent_t gens_ready = nullptr;

    int open(int dev, const HostProveCall& c, size_t host_gen_off, size_t dev_gen_off) {
        BP_RET_ON(hipSetDevice(dev));
        BP_ENGINE_OR_RET(eng);
        e = eng;
        hold = std::unique_lock<std::mutex>(e->prove_host_mu);
        {
            std::lock_guard<std::mutex> lk(e->mu);
            if (!e->stream2) BP_RET_ON(hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking));
            st[0] = e->stream;
            st[1] = e->stream2;
            streams = true;
        }
        const size_t gb = bp::gens_bytes(c.n);
        BP_RET_ON(e->prove_host_pinned.need(host_gen_off + gb));
        BP_RET_ON(e->prove_host_dev.need(dev_gen_off + gb));
        host = e->prove_host_pinned.as<uint8_t>();
        dbuf = e->prove_host_dev.as<uint8_t>();
        bp::pack_gens(host + host_gen_off, c.G->elements, c.H->elements, c.g, c.h, c.n);
        gens = GenView::at(dbuf + dev_gen_off, c.n);
        BP_RET_ON(hipMemcpyAsync(dbuf + dev_gen_off, host + host_gen_off, gb, hipMemcpyHostToDevice, st[0]));
        BP_RET_ON(hipEventCreateWithFlags(&gens_ready, hipEventDisableTiming));
        BP_RET_ON(hipEventRecord(gens_ready, st[0]));
        BP_RET_ON(hipStreamWaitEvent(st[1], gens_ready, 0));
        return HIPBP_OK;
    }
    // how a shard ends: after a failure nothing in flight reads the staging any more, and its message is g_err
    int end(int rc, const std::string& what) {
        if (rc != HIPBP_OK && streams) {
            (void)hipStreamSynchronize(st[0]);
            (void)hipStreamSynchronize(st[1]);
        }
        if (rc != HIPBP_OK) g_err = what;
        return rc;
    }
    ~HostStage() {
        if (gens_ready) (void)hipEventDestroy(gens_ready);
    }
};

// One shard of the seeded prover.  Its chunks alternate over the engine's two streams and two staging
// slots: a slot's previous chunk is unpacked into the caller's structs (after its stream is drained)
// before the slot's next chunk is staged, so one chunk's copies and unpacking run under the other's
// kernels.  Slot layout (pinned host and device alike):
// v | gamma [c] | V A S T1 T2 [c] | taux mu t c x a b [c] | L R [c Lr] | valid [c].
static int prove_host_seeded_shard(int dev, const HostProveCall& c, const std::vector<bp::HostChunk>& chunks,
                                   const bp::HostStop& stop) {
    const size_t n = c.n, FE = bp::FE, Lr = (size_t)log2i(n), nch = chunks.size();
    const size_t CH = chunks[0].c;   // (the plan's chunks are all of this size but for a shorter last one)
    // a slot: v | gamma [CH], then the proof-output layout (bp::OutLayout)
    const size_t slot_bytes = bp::OutLayout{CH, CH, Lr, 2 * CH * FE}.slot_bytes();
    HostStage sg;
    int rc = sg.open(dev, c, 2 * slot_bytes, 2 * slot_bytes);
    std::string what = g_err;
    hipError_t err = hipSuccess;
    auto dev_err = [&](const char* w) {
        rc = HIPBP_ERR_DEVICE;
        what = std::string(w) + ": " + hipGetErrorString(err);
    };
    for (size_t ch = 0; ch < nch + 2 && rc == HIPBP_OK; ch++) {
        const int k = (int)(ch & 1);
        uint8_t* hs = sg.host + k * slot_bytes;
        uint8_t* ds = sg.dbuf + k * slot_bytes;
        if (ch >= 2) {   // the slot's previous chunk: wait for its D2H, hand it to the caller
            const size_t p0 = chunks[ch - 2].c0, pc = chunks[ch - 2].c;
            if ((err = hipStreamSynchronize(sg.st[k])) != hipSuccess) { dev_err("chunk sync"); break; }
            const bp::OutLayout lay{CH, pc, Lr, 2 * CH * FE};
            for (size_t q = 0; q < pc && rc == HIPBP_OK; q++)
                if (!c.own->fill(p0 + q, lay, hs, q, n)) {
                    rc = HIPBP_ERR_DEVICE;
                    what = "Failed to allocate memory for a proof's vectors";
                }
            if (rc != HIPBP_OK) break;
        }
        if (ch >= nch) continue;
        if (stop.raised()) { rc = bp::HOST_SHARD_STOPPED; break; }   // another shard failed: no further chunk
        const size_t c0 = chunks[ch].c0, cc = chunks[ch].c;
        memcpy(hs, c.v + c0, cc * FE);
        memcpy(hs + cc * FE, c.gamma + c0, cc * FE);
        if ((err = hipMemcpyAsync(ds, hs, 2 * cc * FE, hipMemcpyHostToDevice, sg.st[k])) != hipSuccess) { dev_err("chunk H2D"); break; }
        const bp::OutLayout lay{CH, cc, Lr, 2 * CH * FE};
        hipbp_prove_input in{cc, n, (const fe25519*)ds, (const fe25519*)ds + cc, nullptr, nullptr, nullptr};
        hipbp_proof_out out;
        lay.view(ds, &out);
        rc = prove_seeded(&in, c.seed32, chunks[ch].index_base, sg.gens, &out, sg.st[k]);
        if (rc != HIPBP_OK) { what = g_err; break; }
        // one D2H of the slot's output regions, points .. valid[c) (the regions are sized for a full
        // chunk; a short last chunk's arrays sit packed at the front of each)
        if ((err = hipMemcpyAsync(hs + lay.o_pts(), ds + lay.o_pts(), lay.used(), hipMemcpyDeviceToHost, sg.st[k])) != hipSuccess)
            dev_err("chunk D2H");
    }
    return sg.end(rc, what);
}

// One shard of the accepted prover.  A chunk is ONE accepted device call (the retry rounds' fixed
// cost is per call), so its chunks are large (HIPBP_PROVE_HOST_ACCEPT_CHUNK) and lie whole
// in the device buffer: v | gamma [c] | the output layout of C | attempts [C].  The pinned staging
// stays the seeded prover's two slots of `piece` proofs: the inputs go up through them, and the
// finished chunk comes back in pieces that alternate over the two slots and streams, a piece being
// unpacked into the caller's structs while the next one copies.  The chunks themselves run one
// after another: a chunk's last piece is unpacked before the next chunk's device call begins.
// `total`: the device calls' statistics, summed over the chunks.
static int prove_host_accepted_shard(int dev, const HostProveCall& c, const std::vector<bp::HostChunk>& chunks,
                                     const bp::HostStop& stop, AcceptStats* total) {
    const size_t n = c.n, FE = bp::FE, GE = bp::GE, Lr = (size_t)log2i(n);
    const size_t C = chunks[0].c, P = std::min(c.piece, C);
    const auto up = [](size_t b) { return (b + 127) & ~(size_t)127; };
    const size_t o_att = bp::OutLayout{P, P, Lr, 2 * P * FE}.slot_bytes();   // a slot: the seeded prover's, then attempts [P]
    const size_t slot_bytes = o_att + up(P);
    const size_t d_att = bp::OutLayout{C, C, Lr, 2 * C * FE}.slot_bytes(), d_gen = d_att + up(C);
    HostStage sg;
    int rc = sg.open(dev, c, 2 * slot_bytes, d_gen);
    std::string what = g_err;
    hipError_t err = hipSuccess;
    auto dev_err = [&](const char* w) {
        rc = HIPBP_ERR_DEVICE;
        what = std::string(w) + ": " + hipGetErrorString(err);
    };
    uint8_t* ds = sg.dbuf;
    uint8_t* datt = sg.dbuf + d_att;
    for (size_t ch = 0; ch < chunks.size() && rc == HIPBP_OK; ch++) {
        if (stop.raised()) { rc = bp::HOST_SHARD_STOPPED; break; }   // another shard failed: no further chunk
        const size_t c0 = chunks[ch].c0, cc = chunks[ch].c;
        // v | gamma up on stream 0, as many proofs at a time as a slot holds
        const size_t pin_in = slot_bytes / (2 * FE);
        for (size_t p0 = 0, j = 0; p0 < cc; p0 += pin_in, j++) {
            const size_t pc = std::min(pin_in, cc - p0);
            uint8_t* hs = sg.host + (j & 1) * slot_bytes;
            if (j >= 2 && (err = hipStreamSynchronize(sg.st[0])) != hipSuccess) { dev_err("chunk input sync"); break; }
            memcpy(hs, c.v + c0 + p0, pc * FE);
            memcpy(hs + pc * FE, c.gamma + c0 + p0, pc * FE);
            if ((err = hipMemcpyAsync(ds + p0 * FE, hs, pc * FE, hipMemcpyHostToDevice, sg.st[0])) != hipSuccess ||
                (err = hipMemcpyAsync(ds + (cc + p0) * FE, hs + pc * FE, pc * FE, hipMemcpyHostToDevice, sg.st[0])) != hipSuccess) { dev_err("chunk H2D"); break; }
        }
        if (rc != HIPBP_OK) break;
        const bp::OutLayout lay{C, cc, Lr, 2 * C * FE};
        hipbp_prove_input in{cc, n, (const fe25519*)ds, (const fe25519*)ds + cc, nullptr, nullptr, nullptr};
        hipbp_proof_out out;
        lay.view(ds, &out);
        rc = prove_accepted(&in, c.seed32, chunks[ch].index_base, c.max_attempts, c.check, sg.gens, &out, datt, sg.st[0]);
        if (rc != HIPBP_OK) { what = g_err; break; }
        // (the call returned with stream 0 drained: the chunk is complete, the pinned slots are free)
        total->add(g_accept_stats);
        const size_t np = (cc + P - 1) / P;
        for (size_t j = 0; j < np + 2 && rc == HIPBP_OK; j++) {
            const int k = (int)(j & 1);
            uint8_t* hs = sg.host + k * slot_bytes;
            if (j >= 2) {   // the slot's previous piece: wait for its copies, hand it to the caller
                const size_t p0 = (j - 2) * P, pc = std::min(P, cc - p0);
                if ((err = hipStreamSynchronize(sg.st[k])) != hipSuccess) { dev_err("piece sync"); break; }
                const bp::OutLayout pl{P, pc, Lr, 2 * P * FE};
                for (size_t q = 0; q < pc && rc == HIPBP_OK; q++)
                    if (!c.own->fill(c0 + p0 + q, pl, hs, q, n, hs[o_att + q])) {
                        rc = HIPBP_ERR_DEVICE;
                        what = "Failed to allocate memory for a proof's vectors";
                    }
                if (rc != HIPBP_OK) break;
            }
            if (j >= np) continue;
            // rows [p0, p0 + pc) of each of the chunk's arrays, packed at stride pc into the slot
            const size_t p0 = j * P, pc = std::min(P, cc - p0);
            hipbp_proof_out hv;
            bp::OutLayout{P, pc, Lr, 2 * P * FE}.view(hs, &hv);
            err = hipSuccess;
            auto cp = [&](void* dst, const void* src, size_t bytes) {
                if (err == hipSuccess && bytes) err = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, sg.st[k]);
            };
            ge25519* const hp[5] = {hv.V, hv.A, hv.S, hv.T1, hv.T2};
            ge25519* const dp[5] = {out.V, out.A, out.S, out.T1, out.T2};
            for (int i = 0; i < 5; i++) cp(hp[i], dp[i] + p0, pc * GE);
            fe25519* const hf[7] = {hv.taux, hv.mu, hv.t, hv.c, hv.x, hv.a, hv.b};
            fe25519* const df[7] = {out.taux, out.mu, out.t, out.c, out.x, out.a, out.b};
            for (int i = 0; i < 7; i++) cp(hf[i], df[i] + p0, pc * FE);
            if (Lr) {
                cp(hv.L, out.L + p0 * Lr, pc * Lr * GE);
                cp(hv.R, out.R + p0 * Lr, pc * Lr * GE);
            }
            cp(hv.valid, out.valid + p0, pc);
            cp(hs + o_att, datt + p0, pc);
            if (err != hipSuccess) dev_err("piece D2H");
        }
    }
    return sg.end(rc, what);
}

static size_t env_chunk(const char* name, size_t dflt) {   // a chunk size: at most 2^22, the device calls' limit
    size_t ch = dflt;
    if (const char* ce = getenv(name))
        if (atol(ce) > 0) ch = (size_t)atol(ce);
    return std::min(ch, (size_t)1 << 22);
}
// Both host provers: the argument checks (nothing written on an error), the shards' threads, the
// merge.  attempts, max_attempts, check: the accepted prover's (max_attempts = 0: the seeded prover).
static int prove_host_run(RangeProof* proofs, uint8_t* valid, uint8_t* attempts, const fe25519* v, const fe25519* gamma,
                          size_t count, size_t n, const PointVector* G, const PointVector* H, const ge25519* g,
                          const ge25519* h, const uint8_t* seed32, uint64_t index_base, bool accepted, int max_attempts,
                          int check, int num_gpus) {
    if (count == 0) return HIPBP_OK;
    if (!proofs || !valid || !G || !H || !g || !h || !G->elements || !H->elements) {
        g_err = "null argument";
        return HIPBP_ERR_ARG;
    }
    int rc = seed_check(seed32, v, gamma, 0, n);
    if (rc != HIPBP_OK) return rc;
    if (G->length != n || H->length != n) { g_err = "prover: G and H must hold n generators"; return HIPBP_ERR_ARG; }
    if (accepted) {
        if (max_attempts < 1 || max_attempts > 16) { g_err = "accepted prover: max_attempts must be 1..16"; return HIPBP_ERR_ARG; }
        if (check != 1 && check != 2) { g_err = "accepted prover: check must be 1 or 2"; return HIPBP_ERR_ARG; }
        if (!attempts) { g_err = "accepted prover: null attempts"; return HIPBP_ERR_ARG; }
    }
    HostFan fan;
    if ((rc = fan.open(count, num_gpus)) != HIPBP_OK) return rc;
    const size_t chunk = accepted ? env_chunk("HIPBP_PROVE_HOST_ACCEPT_CHUNK", 65536) : env_chunk("HIPBP_PROVE_HOST_CHUNK", 16384);
    if (accepted) g_accept_stats = AcceptStats{};

    bp::ProofOwner own(proofs, valid, attempts, count);   // (zeroes the three outputs)
    const HostProveCall call{v, gamma, n, G, H, g, h, seed32, accepted ? max_attempts : 0, check,
                             env_chunk("HIPBP_PROVE_HOST_CHUNK", 16384), &own};
    std::vector<AcceptStats> stats(fan.ng);   // [shard d]: its device calls', carried back from its thread
    // A call of one shard has the caller's thread for it: the proofs' vectors then come from the
    // caller's malloc arena as they always did; from a thread of its own the one-device seeded call
    // measured 190.7 ms against the parent commit's 180.4 (174.3-184.8), DESIGN §15.
    rc = fan.run(count, [&](int dev, const bp::HostShard& sh, const bp::HostStop& stop) {
        const std::vector<bp::HostChunk> chunks = bp::plan_host_chunks(sh, std::min(chunk, sh.hi - sh.lo), index_base);
        return accepted ? prove_host_accepted_shard(dev, call, chunks, stop, &stats[sh.d])
                        : prove_host_seeded_shard(dev, call, chunks, stop);
    });
    if (rc != HIPBP_OK) {
        own.rollback();   // every vector of every shard freed, proofs, valid and attempts zero
        return rc;
    }
    if (accepted) {
        g_accept_stats = AcceptStats{};   // (a shard run on this thread left its last chunk's here)
        for (const AcceptStats& st : stats) g_accept_stats.add(st);
    }
    return HIPBP_OK;
}

// One shard of the host form on device `dev`: commitments [lo, hi) of the call, in pieces of one
// commit chunk through the device's prove-host staging (h | g | v | gamma | out of a piece; the
// shard keeps prove_host_mu like the host provers' shards, so shards and calls that share a device
// run one after another) on the engine's own stream, each piece drained before the next is staged.
static int commit_host_shard(int dev, ge25519* out, const fe25519* v, const fe25519* gamma, size_t lo, size_t hi,
                             const ge25519* g, const ge25519* h) {
    BP_RET_ON(hipSetDevice(dev));
    BP_ENGINE_OR_RET(e);
    std::unique_lock<std::mutex> hold(e->prove_host_mu);
    const size_t FE = bp::FE, GE = bp::GE;
    const size_t piece = env_commit_chunk(hi - lo);
    hipStream_t s = e->stream;
    BP_RET_ON(hipStreamSynchronize(s));   // (the staging may grow)
    BP_RET_ON(e->prove_host_dev.need(2 * GE + piece * (2 * FE + GE)));
    uint8_t* d = e->prove_host_dev.as<uint8_t>();
    const GenView dg = GenView::at(d, 0);   // (no G, H: the packed h | g)
    const fe25519* dv = (const fe25519*)(d + 2 * GE);
    ge25519* dout = (ge25519*)(d + 2 * GE + 2 * piece * FE);
    BP_RET_ON(hipMemcpyAsync((void*)dg.g, g, GE, hipMemcpyHostToDevice, s));
    BP_RET_ON(hipMemcpyAsync((void*)dg.h, h, GE, hipMemcpyHostToDevice, s));
    for (size_t c0 = lo; c0 < hi; c0 += piece) {
        const size_t c = std::min(piece, hi - c0);
        BP_RET_ON(hipMemcpyAsync((void*)dv, v + c0, c * FE, hipMemcpyHostToDevice, s));
        BP_RET_ON(hipMemcpyAsync((void*)(dv + piece), gamma + c0, c * FE, hipMemcpyHostToDevice, s));
        if (int rc = commit_run(*e, dout, nullptr, nullptr, dv, dv + piece, c, dg, s)) return rc;
        BP_RET_ON(hipMemcpyAsync(out + c0, dout, c * GE, hipMemcpyDeviceToHost, s));
        BP_RET_ON(hipStreamSynchronize(s));
    }
    return HIPBP_OK;
}

// What a shard of the host verifiers takes its 1024-proof chunks from.  host_bytes / dev_bytes: the
// chunk's pinned and device staging; stage: fills the pinned bytes at hc, enqueues on s what leaves the
// flat chunk at dc, and views it as *b, a zeroed batch with its n set (`word`: a zeroed device word of the
// shard's, summed into by a source that counts something); out_index: where proof k of the shard's verdicts goes.
static int chunk_h2d(void* dc, const void* hc, size_t bytes, hipStream_t s) {   // the staged bytes' upload
    const hipError_t err = hipMemcpyAsync(dc, hc, bytes, hipMemcpyHostToDevice, s);
    if (err != hipSuccess) g_err = std::string("chunk H2D: ") + hipGetErrorString(err);
    return err == hipSuccess ? HIPBP_OK : HIPBP_ERR_DEVICE;
}

// The caller's host structs (hipbp_batch_range_proof_verify_host): packed on the host, copied as they are.
struct StructChunks {
    const RangeProof* proofs;
    const ge25519* V;
    const size_t* idx;
    size_t abl, Lr;
    size_t host_bytes(size_t, size_t c) const { return bp::ChunkLayout{c, abl, Lr}.bytes(); }
    size_t dev_bytes(size_t c0, size_t c) const { return host_bytes(c0, c); }
    size_t out_index(size_t k) const { return idx[k]; }
    int stage(size_t c0, size_t c, uint8_t* hc, uint8_t* dc, uint32_t*, hipStream_t s, hipbp_proof_batch* b) const {
        const bp::ChunkLayout lay{c, abl, Lr};
        for (size_t k = 0; k < c; k++) {
            const RangeProof& p = proofs[idx[c0 + k]];
            lay.pack(hc, k, p.ip_proof, &p, &V[idx[c0 + k]]);
        }
        if (int rc = chunk_h2d(dc, hc, lay.bytes(), s)) return rc;
        lay.view(dc, b);
        return HIPBP_OK;
    }
};

static inline size_t pad16(size_t x) { return (x + 15) & ~(size_t)15; }

// A host blob's proofs [lo, lo + B) (hipbp_batch_range_proof_verify_bytes_host; the blob parsed by the
// caller): a chunk uploads its kind bytes, its compact slots, its raw_index entries and raw records
// (raw_index is ascending: two binary searches bound them) and the caller's V rows, each part at a
// 16-byte boundary, and decodes them on the chunk's stream into a flat chunk behind the copy, with
// taux | mu after it when the blob has them.
struct BlobChunks {
    const uint8_t* blob;
    bp::CodecLayout l;   // the whole blob's
    size_t R, lo;
    const ge25519* V;    // the caller's, or null: each proof's own
    struct Parts { size_t j0, nr, o_cmp, o_idx, o_raw, o_v, slice, o_flat, o_tm, end; };
    Parts parts(size_t c0, size_t c) const {
        Parts p;
        const uint8_t* ri = blob + l.o_rawidx();
        p.j0 = bp::codec_raw_lower(ri, R, lo + c0);
        p.nr = bp::codec_raw_lower(ri, R, lo + c0 + c) - p.j0;
        p.o_cmp = pad16(c);
        p.o_idx = p.o_cmp + c * l.Sc();
        p.o_raw = p.o_idx + pad16(4 * p.nr);
        p.o_v = p.o_raw + pad16(p.nr * l.Sr());
        p.slice = p.o_v + (V ? c * bp::GE : 0);
        p.o_flat = (p.slice + 127) & ~(size_t)127;
        p.o_tm = p.o_flat + bp::ChunkLayout{c, l.abl, l.Lr}.bytes();
        p.end = p.o_tm + (l.f ? 2 * c * bp::FE : 0);
        return p;
    }
    size_t host_bytes(size_t c0, size_t c) const { return (parts(c0, c).slice + 127) & ~(size_t)127; }
    size_t dev_bytes(size_t c0, size_t c) const { return (parts(c0, c).end + 127) & ~(size_t)127; }
    size_t out_index(size_t k) const { return lo + k; }
    int stage(size_t c0, size_t c, uint8_t* hc, uint8_t* dc, uint32_t* word, hipStream_t s, hipbp_proof_batch* b) const {
        const Parts p = parts(c0, c);
        const size_t P0 = lo + c0;
        memcpy(hc, blob + l.o_kind() + P0, c);
        memcpy(hc + p.o_cmp, blob + l.o_compact() + P0 * l.Sc(), c * l.Sc());
        memcpy(hc + p.o_idx, blob + l.o_rawidx() + 4 * p.j0, 4 * p.nr);
        memcpy(hc + p.o_raw, blob + l.o_raw(R) + p.j0 * l.Sr(), p.nr * l.Sr());
        if (V) memcpy(hc + p.o_v, V + P0, c * bp::GE);
        if (int rc = chunk_h2d(dc, hc, p.slice, s)) return rc;
        bp::ChunkLayout{c, l.abl, l.Lr}.view(dc + p.o_flat, b);
        b->taux = l.f ? (const fe25519*)(dc + p.o_tm) : nullptr;
        b->mu = l.f ? b->taux + c : nullptr;
        const bp::CodecArrays A = bp::codec_arrays(*b, true, l.f != 0);   // (where the chunk is decoded to)
        if (V) {   // the verify's V argument is the caller's; the proof's own V stays where it was decoded
            b->Vp = b->V;
            b->V = (const ge25519*)(dc + p.o_v);
        }
        bp::BlobView v;
        v.kind = dc; v.compact = dc + p.o_cmp; v.rawidx = dc + p.o_idx; v.raw = dc + p.o_raw;
        v.count = c; v.R = p.nr; v.base = P0;
        v.kind_n = v.compact_n = c; v.rawidx_n = v.raw_n = p.nr;
        bp::launch_codec_decode(v, A, l, word, s);
        if (const hipError_t err = hipGetLastError()) {
            g_err = std::string("chunk decode: ") + hipGetErrorString(err);
            return HIPBP_ERR_DEVICE;
        }
        return HIPBP_OK;
    }
};

// one device's shard of a host verifier (its own host thread): B proofs from `src`.  The shard is cut
// into chunks of CHUNK proofs, each staged as its own little flat batch; each chunk is staged,
// copied and pushed as soon as it is staged (the GPU starts while the host stages the rest), and
// the chunks alternate over two pipelines on two streams, whose ticks fill each other's tails.
// mode 1: cuda_range_proof_verify semantics, with the cached host prefix tables; mode 2:
// range_proof_verify semantics (g read), without tables.
template <class Src>
static int host_shard(int dev, const Src& src, size_t B, size_t n, const PointVector* G, const PointVector* H,
               const ge25519* g, const ge25519* h, int mode, uint8_t* ok) {
    BP_RET_ON(hipSetDevice(dev));
    BP_ENGINE_OR_RET(e);
    constexpr size_t CHUNK = 1024;
    const size_t GE = bp::GE;
    const size_t nch = (B + CHUNK - 1) / CHUNK;
    size_t hsum = 0, dsum = 0;
    for (size_t ch = 0; ch < nch; ch++) {
        const size_t c0 = ch * CHUNK, c = std::min(CHUNK, B - c0);
        hsum += src.host_bytes(c0, c);
        dsum += src.dev_bytes(c0, c);
    }
    // after the chunks: the packed generators, the verdicts, and the source's counter word
    const size_t tail = bp::gens_bytes(n) + pad16(B) + 16;
    const size_t gen_off_h = hsum, gen_off = dsum, ok_off_h = gen_off_h + bp::gens_bytes(n), ok_off = gen_off + bp::gens_bytes(n);
    const size_t bytes_h = hsum + tail, bytes = dsum + tail;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->stream2) BP_RET_ON(hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking));
    hipStream_t st[2] = {e->stream, e->stream2};
    // need() frees a buffer that grows: nothing may still read either
    if ((bytes_h > e->host_pinned.cap && e->host_pinned.p) || bytes > e->host_dev.cap) {
        BP_RET_ON(hipStreamSynchronize(st[0]));
        BP_RET_ON(hipStreamSynchronize(st[1]));
    }
    BP_RET_ON(e->host_pinned.need(bytes_h));
    BP_RET_ON(e->host_dev.need(bytes));
    uint8_t* host = e->host_pinned.as<uint8_t>();
    uint8_t* dbuf = e->host_dev.as<uint8_t>();
    bp::pack_gens(host + gen_off_h, G->elements, H->elements, mode == 2 ? g : nullptr, h, n);
    BP_RET_ON(hipMemcpyAsync(dbuf + gen_off, host + gen_off_h, bp::gens_bytes(n, mode == 2), hipMemcpyHostToDevice, st[0]));
    uint32_t* word = (uint32_t*)(dbuf + ok_off + pad16(B));
    BP_RET_ON(hipMemsetAsync(word, 0, 16, st[0]));
    BP_RET_ON(e->ensure_two((int)n));   // engine stream: ordered before the pipeline's first tick
    const GenView dgen = GenView::at(dbuf + gen_off, n, mode == 2);
    // the generators' prefix tables: reused when this call's generator bytes equal the cached set's
    // (then the pipelines read this call's copy and the tables built from identical bytes)
    int hb = 16;
    if (const char* pb = getenv("HIPBP_HOST_PREFIX_BITS")) hb = std::max(0, std::min(atoi(pb), bp::PREFIX_MAX_BITS));
    if (mode == 2) hb = 0;
    while (hb > 0 && (bp::gens_bytes(n) << hb) > (size_t(5) << 28)) hb--;   // at most 1.25 GB of tables (K = 12 at n = 1024)
    if (hb > 0) {
        const uint8_t* key = host + gen_off_h;
        const size_t kb = bp::gens_bytes(n, false);
        if (e->host_tab_bits != hb || e->host_gens_key.size() != kb || memcmp(e->host_gens_key.data(), key, kb) != 0) {
            e->host_tab_bits = 0;
            e->host_gens_key.clear();
            BP_RET_ON(hipStreamSynchronize(st[0]));   // a previous call's tables are no longer read
            BP_RET_ON(hipStreamSynchronize(st[1]));
            if (e->host_gens.need(bp::gens_bytes(n)) != hipSuccess || e->host_tab.need(bp::gens_bytes(n) << hb) != hipSuccess) {
                (void)hipGetLastError();   // no room for the tables: verify without them
                hb = 0;
            }
        }
        if (hb > 0 && e->host_tab_bits == 0) {
            const GenView gg = GenView::at(e->host_gens.p, n);   // G | H | h, and h again in g's place
            BP_RET_ON(hipMemcpyAsync((void*)gg.G, dgen.G, kb, hipMemcpyDeviceToDevice, st[0]));
            BP_RET_ON(hipMemcpyAsync((void*)gg.g, dgen.h, GE, hipMemcpyDeviceToDevice, st[0]));
            bp::launch_prefix_tables(e->host_tab.as<bp::ge>(), gg.G, gg.H, gg.h, gg.g, (int)n, hb, st[0]);
            BP_RET_ON(hipGetLastError());
            e->host_gens_key.assign(key, key + kb);
            e->host_tab_bits = hb;
        }
    }
    Pipeline* pl[2] = {nullptr, nullptr};
    int rc = HIPBP_OK;
    for (int k = 0; k < 2 && rc == HIPBP_OK; k++) rc = pipeline_for(*e, st[k], std::min(B, CHUNK), (int)n, mode, &pl[k]);
    TableLoan loan(dgen.with_tables(e->host_tab.p, hb), pl[0], pl[1]);   // (a pipeline it did not get: skipped)
    hipEvent_t gens_ready = nullptr;
    if (rc == HIPBP_OK) {   // the second stream waits for the generators' copy (and the zeroed word)
        BP_RET_ON(hipEventCreateWithFlags(&gens_ready, hipEventDisableTiming));
        BP_RET_ON(hipEventRecord(gens_ready, st[0]));
        BP_RET_ON(hipStreamWaitEvent(st[1], gens_ready, 0));
    }
    uint8_t* dok = dbuf + ok_off;
    size_t off_h = 0, off = 0;
    for (size_t ch = 0; ch < nch && rc == HIPBP_OK; ch++) {
        const size_t c0 = ch * CHUNK, c = std::min(CHUNK, B - c0);
        hipbp_proof_batch b{};
        b.n = n;
        if ((rc = src.stage(c0, c, host + off_h, dbuf + off, word, st[ch & 1], &b)) != HIPBP_OK) break;
        rc = pl[ch & 1]->push(&b, nullptr, dok + c0, nullptr, nullptr);
        off_h += src.host_bytes(c0, c);
        off += src.dev_bytes(c0, c);
    }
    for (int k = 0; k < 2 && rc == HIPBP_OK; k++) rc = pl[k]->flush();
    hipError_t s1 = hipStreamSynchronize(st[1]);
    if (rc == HIPBP_OK && s1 == hipSuccess) {
        if ((err = hipMemcpyAsync(host + ok_off_h, dok, pad16(B) + 16, hipMemcpyDeviceToHost, st[0])) == hipSuccess)
            err = hipStreamSynchronize(st[0]);
        if (err != hipSuccess) { g_err = std::string("shard D2H: ") + hipGetErrorString(err); rc = HIPBP_ERR_DEVICE; }
        else if (*(const uint32_t*)(host + ok_off_h + pad16(B)) != 0) {   // (the blob was parsed: not reached)
            g_err = "blob decode skipped records of a parsed blob (internal)";
            rc = HIPBP_ERR_DEVICE;
        }
    } else {
        (void)hipStreamSynchronize(st[0]);   // nothing in flight reads the staging any more
        if (rc == HIPBP_OK) { g_err = std::string("stream2: ") + hipGetErrorString(s1); rc = HIPBP_ERR_DEVICE; }
    }
    if (gens_ready) (void)hipEventDestroy(gens_ready);
    if (rc == HIPBP_OK)
        for (size_t k = 0; k < B; k++) ok[src.out_index(k)] = host[ok_off_h + k] ? 1 : 0;
    return rc;
}

// the shape checks of the device batch (n a power of two, L_len <= log2 n) for a host batch
static int host_verify_shape(size_t n, size_t abl, size_t Lr) {
    hipbp_proof_batch probe;
    memset(&probe, 0, sizeof probe);
    probe.count = 1; probe.n = n; probe.ab_len = abl; probe.L_len = Lr;
    const uint8_t dummy[1] = {0};
    probe.V = probe.A = probe.S = probe.T1 = probe.T2 = (const ge25519*)dummy;
    probe.t = probe.a = probe.b = probe.c = probe.x = (const fe25519*)dummy;
    probe.L = probe.R = (const ge25519*)dummy;
    return check_batch(&probe, 1);
}

}  // namespace

extern "C" {

int hipbp_batch_generate_range_proof_host_sharded(RangeProof* proofs, uint8_t* valid, const fe25519* v,
                                                  const fe25519* gamma, size_t count, size_t n, const PointVector* G,
                                                  const PointVector* H, const ge25519* g, const ge25519* h,
                                                  const uint8_t seed32[32], uint64_t index_base, int num_gpus) {
    return prove_host_run(proofs, valid, nullptr, v, gamma, count, n, G, H, g, h, seed32, index_base, false, 0, 0,
                          num_gpus);
}

int hipbp_batch_generate_range_proof_host(RangeProof* proofs, uint8_t* valid, const fe25519* v, const fe25519* gamma,
                                          size_t count, size_t n, const PointVector* G, const PointVector* H,
                                          const ge25519* g, const ge25519* h, const uint8_t seed32[32],
                                          uint64_t index_base) {
    return hipbp_batch_generate_range_proof_host_sharded(proofs, valid, v, gamma, count, n, G, H, g, h, seed32,
                                                         index_base, 1);
}

int hipbp_batch_generate_range_proof_accepted_host(RangeProof* proofs, uint8_t* valid, uint8_t* attempts,
                                                   const fe25519* v, const fe25519* gamma, size_t count, size_t n,
                                                   const PointVector* G, const PointVector* H, const ge25519* g,
                                                   const ge25519* h, const uint8_t seed32[32], uint64_t index_base,
                                                   int max_attempts, int check, int num_gpus) {
    return prove_host_run(proofs, valid, attempts, v, gamma, count, n, G, H, g, h, seed32, index_base, true,
                          max_attempts, check, num_gpus);
}

int hipbp_batch_pedersen_commit_host(ge25519* out, const fe25519* v, const fe25519* gamma, size_t count,
                                     const ge25519* g, const ge25519* h, int num_gpus) {
    if (count == 0) return HIPBP_OK;
    if (!out || !v || !gamma || !g || !h) { g_err = "null argument"; return HIPBP_ERR_ARG; }
    HostFan fan;
    if (int rc = fan.open(count, num_gpus)) return rc;
    return fan.run(count, [&](int dev, const bp::HostShard& sh, const bp::HostStop&) {
        return commit_host_shard(dev, out, v, gamma, sh.lo, sh.hi, g, h);
    });
}

int hipbp_batch_range_proof_verify_host(const RangeProof* proofs, const ge25519* V, size_t count, size_t n,
                                        const PointVector* G, const PointVector* H, const ge25519* g,
                                        const ge25519* h, int num_gpus, uint8_t* ok) {
    (void)g;   // g is not read by cuda_range_proof_verify (crv:82-127)
    if (count == 0) return HIPBP_OK;
    if (!proofs || !V || !G || !H || !h || !ok || !G->elements || !H->elements) {
        g_err = "null argument";
        return HIPBP_ERR_ARG;
    }
    HostFan fan;
    int rc = fan.open(count, num_gpus);
    if (rc != HIPBP_OK) return rc;
    // The flat batch needs one (a/b length, rounds) shape: the first proof that passes the checks
    // sets it (the reference prover's proofs all share it); proofs of another shape go one by one.
    size_t abl = 0, Lr = 0;
    std::vector<size_t> main, other;
    main.reserve(count);
    for (size_t i = 0; i < count; i++) {
        const InnerProductProof& ip = proofs[i].ip_proof;
        ok[i] = 0;
        if (G->length != ip.n || H->length != ip.n || n != ip.n) {   // crv:140-143, as the single call
            fprintf(stderr, "Error: Vector lengths must match for inner product verification\n");
            continue;
        }
        if (ip.b.length != ip.a.length || ip.a.length == 0 || ip.L.length < ip.L_len || ip.R.length < ip.L_len ||
            !ip.a.elements || !ip.b.elements || (ip.L_len && (!ip.L.elements || !ip.R.elements)))
            continue;   // stage_single's check: the single call returns false as well
        if (main.empty()) { abl = ip.a.length; Lr = ip.L_len; }
        (ip.a.length == abl && ip.L_len == Lr ? main : other).push_back(i);
    }
    if (!main.empty() && (rc = host_verify_shape(n, abl, Lr)) != HIPBP_OK) return rc;
    // (the shards: as many as `count` asks for, cut from the index list)
    rc = fan.run(main.size(), [&](int dev, const bp::HostShard& sh, const bp::HostStop&) {
        return host_shard(dev, StructChunks{proofs, V, main.data() + sh.lo, abl, Lr}, sh.hi - sh.lo, n, G, H, nullptr, h, 1, ok);
    });
    if (rc != HIPBP_OK) return rc;
    for (size_t i : other)
        ok[i] = verify_single(&proofs[i].ip_proof, &proofs[i], &V[i], nullptr, n, G, H, h) ? 1 : 0;
    return HIPBP_OK;
}

int hipbp_batch_range_proof_verify_bytes_host(const uint8_t* blob, size_t bytes, const ge25519* V, size_t n,
                                              const PointVector* G, const PointVector* H, const ge25519* g,
                                              const ge25519* h, int check, int num_gpus, uint8_t* ok) {
    const char* me = "range_proof_verify_bytes_host";
    if (check != 1 && check != 2) return codec_fail(me, "check must be 1 or 2");
    hipbp_proof_blob_info info;
    if (const char* e = bp::codec_parse(blob, bytes, &info)) return codec_fail(me, e);   // before anything is uploaded
    if (info.n != n) return codec_fail(me, "n differs from the blob header's");
    if (!G || !H || !h || !G->elements || !H->elements || (info.count && !ok)) return codec_fail(me, "null argument");
    if (G->length != n || H->length != n) return codec_fail(me, "G and H must have n generators");
    if (check == 2 && !(info.flags & 1)) return codec_fail(me, "check 2 needs a blob with taux and mu");
    if (check == 2 && !g) return codec_fail(me, "check 2 needs g");
    if (info.count == 0) return HIPBP_OK;
    int rc = host_verify_shape(n, info.ab_len, info.L_len);
    if (rc != HIPBP_OK) return rc;
    HostFan fan;
    if ((rc = fan.open(info.count, num_gpus)) != HIPBP_OK) return rc;
    const bp::CodecLayout l = bp::codec_layout(info);
    return fan.run(info.count, [&](int dev, const bp::HostShard& sh, const bp::HostStop&) {
        return host_shard(dev, BlobChunks{blob, l, info.raw_count, sh.lo, V}, sh.hi - sh.lo, n, G, H, g, h, check, ok);
    });
}

}  // extern "C"
