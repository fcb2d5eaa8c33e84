// Host-only driver of csrc/rrt_march_cache.h for tests/test_march_cache_host.py: reads commands from stdin, prints what the
// policy decided.  Keys are synthetic: "k <id>" makes key <id> current (ids differ in one field chosen by id).
//   launch <id>        -> action (0 today, 1 fill, 2 replay); a pending fill must be verified first, as the library does
//   verify <0|1>       -> fill_verified(complete)
//   failed <why>       -> fill_failed(why)
//   reset
//   canon <use_lens> <distortion_bits> <nudge_ulps> <nudge_seed> <volumetrics>  -> the canonical fields
//   blocks <rays> <in_block_bytes> <grown> <budget> <fixed> <block_bytes>       -> wanted, in-budget
// Every command prints one line: its result, then state why fills hits drops misses uncacheable.
#include <cstdio>
#include <cstring>
#include <string>
#include <iostream>
#include <sstream>

#include "../../relativisticraytracer_amd/csrc/rrt_march_cache.h"

using namespace rrt_mc;

static MarchKey make(int id) {
    MarchKey k;
    memset(&k, 0, sizeof(k));
    k.width = 64; k.height = 32; k.n_local_rows = 32; k.tile_rows = 32; k.n_shards = 1; k.max_steps = 2000; k.volumetrics = 1;
    // id 0 is the base key; id n > 0 differs from it in 32-bit word (n - 1) of the struct, by one
    if (id > 0) reinterpret_cast<uint32_t*>(&k)[(id - 1) % (sizeof(MarchKey) / 4)] += 1u;
    return k;
}

int main() {
    Policy p;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        long long r = -1, r2 = -1;
        if (cmd == "launch") { int id; in >> id; r = p.next(make(id)); }
        else if (cmd == "pending") { int id; in >> id; r = p.pending_for(make(id)) ? 1 : 0; }
        else if (cmd == "verify") { int ok; in >> ok; p.fill_verified(ok != 0); r = 0; }
        else if (cmd == "failed") { int why; in >> why; p.fill_failed(why); r = 0; }
        else if (cmd == "reset") { p.reset(); r = 0; }
        else if (cmd == "same") { int a, b; in >> a >> b; r = same_key(make(a), make(b)) ? 1 : 0; }
        else if (cmd == "canon") {
            MarchKey k = make(0);
            unsigned d, s; in >> k.use_lens >> d >> k.nudge_ulps >> s >> k.volumetrics;
            k.distortion_amount = d; k.nudge_seed = s;
            canonicalize(k);
            printf("%d %u %d %u %d\n", k.use_lens, k.distortion_amount, k.nudge_ulps, k.nudge_seed, k.volumetrics);
            continue;
        } else if (cmd == "blocks") {
            unsigned long long rays, inb, grown, budget, fixed, bb;
            in >> rays >> inb >> grown >> budget >> fixed >> bb;
            r = (long long)wanted_blocks(rays, inb, grown != 0);
            r2 = (long long)blocks_in_budget((uint64_t)r, budget, fixed, bb);
            printf("%lld %lld\n", r, r2);
            continue;
        } else if (cmd == "words") { printf("%zu\n", sizeof(MarchKey) / 4); continue; }
        else continue;
        printf("%lld %d %d %llu %llu %llu %llu %llu\n", r, p.state, p.why, (unsigned long long)p.st.fills, (unsigned long long)p.st.hits,
               (unsigned long long)p.st.drops, (unsigned long long)p.st.misses, (unsigned long long)p.st.uncacheable);
    }
    return 0;
}
