// bp_host_prove.h — the host-data entry points' shard contract and the host provers' plan and result
// owner (internal to the library): the parts of the host verifiers, provers and commitments that no
// GPU run exercises, the shard count, the split of a call into shards and chunks, the shards' threads
// with the merge of their results, and the rollback after a failure.  Host-only and pure: no HIP
// runtime calls, so tests/host_prove_check.hip runs them all on a CPU.
#pragma once
#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "bp_layout.h"

namespace bp {

// ------------------------------------------------------------------ the plan
// Shard d of ng proves the contiguous block [count d / ng, count (d + 1) / ng): the blocks cover
// [0, count) in order and their sizes differ by at most one.  Empty blocks (ng > count) are left out:
// they start no thread.
struct HostShard {
    int d;
    size_t lo, hi;
};
inline std::vector<HostShard> plan_host_shards(size_t count, int ng) {
    std::vector<HostShard> out;
    for (int d = 0; d < ng; d++) {
        const size_t lo = count * (size_t)d / (size_t)ng, hi = count * (size_t)(d + 1) / (size_t)ng;
        if (hi > lo) out.push_back(HostShard{d, lo, hi});
    }
    return out;
}

// How every host-data entry point reads num_gpus (count >= 1 proofs, ndev devices visible, env =
// HIPBP_HOST_SHARDS's value or null): num_gpus >= 1 asks for that many shards and is an error beyond
// ndev; num_gpus <= 0 takes every visible device, or env's k >= 1 shards, at most 64 and one per
// proof (more shards than devices share them in turn: the split also runs on a one-GPU box).
inline int resolve_host_shards(int num_gpus, int ndev, const char* env, size_t count, int* ng, std::string* err) {
    if (ndev <= 0) { *err = "no HIP device"; return HIPBP_ERR_DEVICE; }
    if (num_gpus > ndev) {   // asked for more devices than are visible: an error, not a silent fallback
        *err = "num_gpus = " + std::to_string(num_gpus) + " but " + std::to_string(ndev) + " HIP device(s) visible";
        return HIPBP_ERR_ARG;
    }
    *ng = num_gpus <= 0 ? ndev : num_gpus;
    if (num_gpus <= 0 && env && atoi(env) > 0) *ng = (int)std::min<size_t>(std::min(atoi(env), 64), count);
    return HIPBP_OK;
}

// ------------------------------------------------------------------ the fan-out
// The flag a fan-out's shards share: raised once a shard has failed on its own, polled by the
// others between chunks; a shard that gives up for it returns HOST_SHARD_STOPPED.
class HostStop {
    std::atomic<bool> up_{false};

  public:
    bool raised() const { return up_.load(); }
    void raise() { up_.store(true); }
};
constexpr int HOST_SHARD_STOPPED = INT_MIN;   // (no return code of the library's)

// run(shard, stop, err) -> return code, once per shard, each on a thread of its own; a call of one
// shard with d = 0 (the caller's device) has the caller's thread for it.  `err` is the shard's own
// message slot (the library's last-error string is per thread).  Every thread is joined before any
// result is read.  Returns the first failure in shard order that is a shard's own, not a stop after
// another's (one exists whenever any shard stopped: only such a failure raises the flag); k ==
// shards.size(): none.
struct HostFanFailure {
    size_t k;
    int rc;
    std::string err;
};
template <class Run>
HostFanFailure host_fanout(const std::vector<HostShard>& shards, Run run) {
    const size_t ns = shards.size();
    HostStop stop;
    std::vector<int> rcs(ns, HIPBP_OK);
    std::vector<std::string> errs(ns);
    auto own_failure = [&](size_t k) { return rcs[k] != HIPBP_OK && rcs[k] != HOST_SHARD_STOPPED; };
    auto one = [&](size_t k) {
        rcs[k] = run(shards[k], (const HostStop&)stop, errs[k]);
        if (own_failure(k)) stop.raise();
    };
    if (ns == 1 && shards[0].d == 0) {
        one(0);
    } else {
        std::vector<std::thread> workers;
        for (size_t k = 0; k < ns; k++) workers.emplace_back(one, k);
        for (auto& w : workers) w.join();
    }
    for (size_t k = 0; k < ns; k++)
        if (own_failure(k)) return HostFanFailure{k, rcs[k], errs[k]};
    return HostFanFailure{ns, HIPBP_OK, std::string()};
}

// A shard's chunks, in order: proofs [c0, c0 + c) of the call, c = chunk but for a shorter last one,
// proved with the chunk's own index_base = the call's + c0 (mod 2^64: the global index of proof c0),
// so every proof keeps the index it has in the unsplit call.
struct HostChunk {
    size_t c0, c;
    uint64_t index_base;
};
inline std::vector<HostChunk> plan_host_chunks(const HostShard& sh, size_t chunk, uint64_t index_base) {
    std::vector<HostChunk> out;
    if (chunk == 0) chunk = 1;
    for (size_t c0 = sh.lo; c0 < sh.hi; c0 += chunk) {
        const size_t c = sh.hi - c0 < chunk ? sh.hi - c0 : chunk;
        out.push_back(HostChunk{c0, c, index_base + (uint64_t)c0});
    }
    return out;
}

// ------------------------------------------------------------------ the result owner
// What hands a call's results to the caller: proofs[count], valid[count] and (the accepted prover)
// attempts[count], all zeroed at construction, and the record of which proofs[i] may own vectors
// from `al.alloc`.  fill() is called by the shard threads, each for the proofs of its own block: proof
// i's mark is a byte of its own, written by that one thread before the first allocation for i and
// read by rollback() only after every thread was joined, so the owner needs no lock.
struct HostAlloc {
    AllocFn alloc;
    void (*release)(void*);
};
inline HostAlloc host_malloc() { return HostAlloc{malloc, free}; }

class ProofOwner {
    RangeProof* proofs_;
    uint8_t *valid_, *attempts_;   // attempts_: null for the seeded prover
    size_t count_;
    HostAlloc al_;
    std::unique_ptr<uint8_t[]> owns_;   // [count]: proofs[i] may hold allocated vectors

    void clear() {
        memset(proofs_, 0, count_ * sizeof(RangeProof));
        memset(valid_, 0, count_);
        if (attempts_) memset(attempts_, 0, count_);
    }

  public:
    ProofOwner(RangeProof* proofs, uint8_t* valid, uint8_t* attempts, size_t count, HostAlloc al = host_malloc())
        : proofs_(proofs), valid_(valid), attempts_(attempts), count_(count), al_(al), owns_(new uint8_t[count]()) {
        clear();
    }
    // proofs[i], valid[i] (and attempts[i] = att) from row k of a host copy `base` of an output
    // layout, n = 1 << lay.Lr.  False: an allocation failed (proofs[i] owns what it got: roll back).
    bool fill(size_t i, const OutLayout& lay, const void* base, size_t k, size_t n, uint8_t att = 0) {
        owns_[i] = 1;
        const int v = lay.unpack(base, k, n, proofs_[i], al_.alloc);
        if (v < 0) return false;
        valid_[i] = (uint8_t)v;
        if (attempts_) attempts_[i] = att;
        return true;
    }
    // After a failure in any shard, every thread joined: every vector handed out is released and
    // every output byte is zero again.
    void rollback() {
        for (size_t i = 0; i < count_; i++) {
            if (!owns_[i]) continue;
            InnerProductProof& ip = proofs_[i].ip_proof;
            al_.release(ip.a.elements); al_.release(ip.b.elements);
            al_.release(ip.L.elements); al_.release(ip.R.elements);
            owns_[i] = 0;
        }
        clear();
    }
};

}  // namespace bp
