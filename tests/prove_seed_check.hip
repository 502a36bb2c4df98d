// prove_seed_check.hip — the seeded prover's derivation (csrc/bp_prove_seed.h) compiled as HOST code
// (hipcc --cuda-host-only) and printed for tests/test_prove_seed_host.py to compare with hashlib.
//
//   prove_seed_check CASE...      CASE = seed:v:gamma:index:n:slots
//
// seed, v, gamma: 64 hex digits, the 32 bytes in memory order (v, gamma: the four LE u64 limbs);
// index: decimal u64 (index_base + p, already summed); n: decimal; slots: "all" or a comma list.
// Per case: "key <64 hex>" then one "slot <k> <limb0> <limb1> <limb2> <limb3>" line per slot.
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

int main(int argc, char** argv) {
    for (int a = 1; a < argc; a++) {
        std::vector<std::string> f;
        std::string cur;
        for (const char* p = argv[a];; p++) {
            if (*p == ':' || *p == 0) {
                f.push_back(cur);
                cur.clear();
                if (*p == 0) break;
            } else {
                cur += *p;
            }
        }
        uint8_t seed[32], vb[32], gb[32];
        if (f.size() != 6 || !unhex(f[0], seed) || !unhex(f[1], vb) || !unhex(f[2], gb)) {
            fprintf(stderr, "bad case %s\n", argv[a]);
            return 2;
        }
        uint64_t v[4], g[4], key[4];
        limbs(vb, v);
        limbs(gb, g);
        const uint64_t index = strtoull(f[3].c_str(), nullptr, 10);
        const uint32_t n = (uint32_t)strtoul(f[4].c_str(), nullptr, 10);
        bp::seed_key(key, bp::seed_words(seed), v, g, index, n);
        printf("key ");
        for (int i = 0; i < 4; i++)
            for (int k = 0; k < 8; k++) printf("%02x", (unsigned)(key[i] >> (8 * k) & 0xff));
        printf("\n");
        std::vector<uint32_t> slots;
        if (f[5] == "all") {
            for (uint32_t s = 0; s < 2 * n + 4; s++) slots.push_back(s);
        } else {
            for (char* p = &f[5][0]; *p;) {
                slots.push_back((uint32_t)strtoul(p, &p, 10));
                if (*p == ',') p++;
            }
        }
        for (uint32_t s : slots) {
            uint64_t d[4];
            bp::seed_scalar(d, key, s);
            printf("slot %u %016llx %016llx %016llx %016llx\n", s, (unsigned long long)d[0], (unsigned long long)d[1],
                   (unsigned long long)d[2], (unsigned long long)d[3]);
        }
    }
    return 0;
}
