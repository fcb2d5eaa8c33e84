// Host-only driver of csrc/rrt_handles.h for tests/test_handles_host.py.  Each case is a command-line word; a case prints
// "<case> ok" and exits 0, or says which expectation failed and exits 1.
//   ids       ids are issued from the given start (both id types the library uses) and never reused after take
//   unknown   get and take of an unknown id fail and leave the table as it was
//   refuse    take with a rejecting predicate leaves the element registered; an accepting one then gets it
//   pinned    a shared_ptr element obtained by get outlives another caller's take
//   threads   8 threads x 10 000 mixed insert / get / take: the expected element count, no id issued twice
#include <atomic>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>
#include <algorithm>

#include "../../relativisticraytracer_amd/csrc/rrt_handles.h"

using namespace rrt_handles;

#define EXPECT(cond)                                                                    \
    do { if (!(cond)) { fprintf(stderr, "handle exerciser: %s failed (line %d)\n", #cond, __LINE__); return 1; } } while (0)

struct Thing { int value; int device; };

static int case_ids() {
    HandleTable<unsigned long long, Thing> big(0x5254000000000001ull);
    HandleTable<int, Thing> small(1);
    EXPECT(big.insert(Thing{7, 0}) == 0x5254000000000001ull && big.insert(Thing{8, 0}) == 0x5254000000000002ull);
    Thing t{0, 0};
    for (int k = 1; k <= 5; ++k) EXPECT(small.insert(Thing{10 * k, 0}) == k);
    EXPECT(small.take(2, t) == kTaken && t.value == 20 && small.take(5, t) == kTaken && t.value == 50);
    EXPECT(small.insert(Thing{60, 0}) == 6 && small.insert(Thing{70, 0}) == 7);      // neither 2 nor 5 again
    EXPECT(!small.get(2, t) && !small.get(5, t) && small.get(6, t) && t.value == 60);
    for (int k : {1, 3, 4, 6, 7}) EXPECT(small.take(k, t) == kTaken);
    EXPECT(small.size() == 0 && small.insert(Thing{80, 0}) == 8);                    // an emptied table does not start over
    EXPECT(big.take(0x5254000000000001ull, t) == kTaken && big.insert(Thing{9, 0}) == 0x5254000000000003ull);
    return 0;
}

static int case_unknown() {
    HandleTable<int, Thing> tab(1);
    const int id = tab.insert(Thing{5, 3});
    Thing t{-1, -1};
    for (int stale : {0, -1, 2, 4242, 12345}) {
        EXPECT(!tab.get(stale, t) && t.value == -1);
        EXPECT(tab.take(stale, t) == kUnknown && t.value == -1);
        EXPECT(tab.take(stale, t, [](const Thing&) { return false; }) == kUnknown);
    }
    EXPECT(tab.size() == 1 && tab.get(id, t) && t.value == 5 && t.device == 3);
    EXPECT(tab.insert(Thing{6, 3}) == id + 1);           // a failed lookup issues no id
    return 0;
}

static int case_refuse() {
    HandleTable<int, std::shared_ptr<Thing>> tab(1);
    const int id = tab.insert(std::make_shared<Thing>(Thing{11, 2}));
    std::shared_ptr<Thing> got;
    int asked = 0;
    EXPECT(tab.take(id, got, [&](const std::shared_ptr<Thing>& p) { ++asked; return p->device == 5; }) == kRefused);
    EXPECT(asked == 1 && !got && tab.size() == 1);
    EXPECT(tab.get(id, got) && got->value == 11);        // still registered
    got.reset();
    EXPECT(tab.take(id, got, [&](const std::shared_ptr<Thing>& p) { ++asked; return p->device == 2; }) == kTaken);
    EXPECT(asked == 2 && got && got->value == 11 && tab.size() == 0);
    EXPECT(tab.take(id, got) == kUnknown);               // destroy twice
    return 0;
}

static int case_pinned() {
    static std::atomic<int> alive{0};
    struct Counted { int v = 3; Counted() { ++alive; } ~Counted() { --alive; } };
    HandleTable<int, std::shared_ptr<Counted>> tab(1);
    const int id = tab.insert(std::make_shared<Counted>());
    std::shared_ptr<Counted> user, owner;
    EXPECT(tab.get(id, user) && alive == 1);
    EXPECT(tab.take(id, owner) == kTaken && owner == user);
    owner.reset();                                       // the destroying caller lets go ...
    EXPECT(alive == 1 && user->v == 3 && !tab.get(id, owner));       // ... the launch's copy still holds the object
    user.reset();
    EXPECT(alive == 0);
    return 0;
}

static int case_threads() {
    constexpr int kThreads = 8, kOps = 10000;
    HandleTable<int, std::shared_ptr<Thing>> tab(1);
    std::vector<std::vector<int>> issued(kThreads);
    std::atomic<long long> inserted{0}, taken{0};
    std::atomic<int> bad{0};
    std::vector<std::thread> pool;
    for (int w = 0; w < kThreads; ++w)
        pool.emplace_back([&, w] {
            unsigned rng = 12345u + 977u * (unsigned)w;
            std::vector<int> mine;
            for (int k = 0; k < kOps; ++k) {
                rng = rng * 1664525u + 1013904223u;
                const unsigned op = (rng >> 16) % 4u;
                if (op <= 1u || mine.empty()) {                   // insert
                    const int id = tab.insert(std::make_shared<Thing>(Thing{w, 0}));
                    mine.push_back(id); issued[w].push_back(id); ++inserted;
                } else if (op == 2u) {                            // get: an id of its own, or (often unknown) a neighbour's guess
                    std::shared_ptr<Thing> p;
                    const int id = mine[(rng >> 8) % mine.size()];
                    if (!tab.get(id, p) || p->value != w) ++bad;
                    (void)tab.get(id + 1 + (int)(rng % 97u), p);
                } else {                                          // take: refused once, then for real
                    std::shared_ptr<Thing> p;
                    const size_t at = (rng >> 8) % mine.size();
                    if (tab.take(mine[at], p, [](const std::shared_ptr<Thing>&) { return false; }) != kRefused) ++bad;
                    if (tab.take(mine[at], p) != kTaken || p->value != w) ++bad;
                    if (tab.take(mine[at], p) != kUnknown) ++bad;
                    mine[at] = mine.back(); mine.pop_back(); ++taken;
                }
            }
        });
    for (auto& t : pool) t.join();
    EXPECT(bad == 0);
    EXPECT((long long)tab.size() == inserted - taken);
    std::vector<int> all;
    for (const auto& v : issued) all.insert(all.end(), v.begin(), v.end());
    std::sort(all.begin(), all.end());
    EXPECT((long long)all.size() == inserted && std::adjacent_find(all.begin(), all.end()) == all.end());
    EXPECT(all.front() == 1 && all.back() == (int)all.size());       // 1 .. n, each once
    return 0;
}

int main(int argc, char** argv) {
    for (int k = 1; k < argc; ++k) {
        int rc = 2;
        if (!strcmp(argv[k], "ids")) rc = case_ids();
        else if (!strcmp(argv[k], "unknown")) rc = case_unknown();
        else if (!strcmp(argv[k], "refuse")) rc = case_refuse();
        else if (!strcmp(argv[k], "pinned")) rc = case_pinned();
        else if (!strcmp(argv[k], "threads")) rc = case_threads();
        if (rc != 0) { if (rc == 2) fprintf(stderr, "handle exerciser: unknown case %s\n", argv[k]); return 1; }
        printf("%s ok\n", argv[k]);
    }
    return 0;
}
