// prove_try_check.hip — the accepted prover's retry derivation (csrc/bp_prove_seed.h: seed_try_key
// on top of seed_key and seed_scalar) compiled as HOST code (hipcc --cuda-host-only) and printed for
// tests/test_prove_try_host.py to compare with hashlib.
//
//   prove_try_check CASE...      CASE = seed:v:gamma:index:n:a:slots
//
// seed, v, gamma: 64 hex digits, the 32 bytes in memory order (v, gamma: the four LE u64 limbs);
// index: decimal u64 (index_base + p, already summed); n: decimal; a: decimal u32, the attempt;
// slots: a comma list (may be empty).
// Per case: "key <64 hex>" (key_p), "try <64 hex>" (key_{p,a}), then one
// "slot <k> <limb0> <limb1> <limb2> <limb3>" line per slot, under key_{p,a}.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../cudabulletproof_amd/csrc/bp_prove_seed.h"

static bool unhex(const std::string& s, uint8_t out[32]) {
    if (s.size() != 64) return false;
    for (int i = 0; i < 32; i++) {
        unsigned x;
        if (sscanf(s.c_str() + 2 * i, "%2x", &x) != 1) return false;
        out[i] = (uint8_t)x;
    }
    return true;
}

static void limbs(const uint8_t b[32], uint64_t v[4]) {
    for (int i = 0; i < 4; i++) {
        v[i] = 0;
        for (int k = 7; k >= 0; k--) v[i] = v[i] << 8 | b[8 * i + k];
    }
}

static void print_key(const char* what, const uint64_t key[4]) {
    printf("%s ", what);
    for (int i = 0; i < 4; i++)
        for (int k = 0; k < 8; k++) printf("%02x", (unsigned)(key[i] >> (8 * k) & 0xff));
    printf("\n");
}

int main(int argc, char** argv) {
    for (int c = 1; c < argc; c++) {
        std::vector<std::string> f;
        std::string cur;
        for (const char* p = argv[c];; p++) {
            if (*p == ':' || *p == 0) {
                f.push_back(cur);
                cur.clear();
                if (*p == 0) break;
            } else {
                cur += *p;
            }
        }
        uint8_t seed[32], vb[32], gb[32];
        if (f.size() != 7 || !unhex(f[0], seed) || !unhex(f[1], vb) || !unhex(f[2], gb)) {
            fprintf(stderr, "bad case %s\n", argv[c]);
            return 2;
        }
        uint64_t v[4], g[4], key[4], tkey[4];
        limbs(vb, v);
        limbs(gb, g);
        const uint64_t index = strtoull(f[3].c_str(), nullptr, 10);
        const uint32_t n = (uint32_t)strtoul(f[4].c_str(), nullptr, 10);
        const uint32_t a = (uint32_t)strtoul(f[5].c_str(), nullptr, 10);
        bp::seed_key(key, bp::seed_words(seed), v, g, index, n);
        bp::seed_try_key(tkey, key, a);
        print_key("key", key);
        print_key("try", tkey);
        for (char* p = &f[6][0]; *p;) {
            const uint32_t s = (uint32_t)strtoul(p, &p, 10);
            if (*p == ',') p++;
            uint64_t d[4];
            bp::seed_scalar(d, tkey, s);
            printf("slot %u %016llx %016llx %016llx %016llx\n", s, (unsigned long long)d[0], (unsigned long long)d[1],
                   (unsigned long long)d[2], (unsigned long long)d[3]);
        }
    }
    return 0;
}
