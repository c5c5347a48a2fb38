// pf_launch.h — the launch half of pathfeas.hip that makes no HIP call: the check of a call's
// set_ids, the order a call's sets are launched in, the launch geometry (candidates per wave,
// items, waves, blocks), the sum of the counter lines and the 256-byte alignment of every block
// layout.  pathfeas.hip keeps the knobs' globals, streams, blocks, launches and copies and passes
// the numbers in.  Host only (tests/host_launch_check.cpp builds it with the host compiler);
// pf_devprog.h's style: static inline, errors as std::string.
#ifndef PF_LAUNCH_H
#define PF_LAUNCH_H

#include "pf_devprog.h"

namespace pf_launch {

using pf_devprog::errorf;

// every region of a device block starts 256-byte aligned
static inline size_t al(size_t b) { return (b + 255) & ~size_t(255); }

// ---- a call's set_ids ----------------------------------------------------------------------
// Every id below n_sets and none requested twice; `also(set)` is the entry point's own per-set
// condition (an error message, empty when it holds), asked after those two.  Empty: accepted.
template <typename Also>
static inline std::string check_request(const char* who, size_t n_sets, const uint32_t* set_ids, size_t n, Also also) {
    if (n && !set_ids) return errorf("%s: null set_ids", who);
    std::vector<uint8_t> seen(n_sets, 0);
    for (size_t i = 0; i < n; i++) {
        const uint32_t s = set_ids[i];
        if (s >= n_sets) return errorf("%s: set %u out of range (%zu sets)", who, s, n_sets);
        if (seen[s]) return errorf("%s: set %u requested twice", who, s);
        std::string e = also(s);
        if (!e.empty()) return e;
        seen[s] = 1;
    }
    return std::string();
}
static inline std::string check_request(const char* who, size_t n_sets, const uint32_t* set_ids, size_t n) {
    return check_request(who, n_sets, set_ids, n, [](uint32_t) { return std::string(); });
}

// a launch's work-queue items are numbered in 32 bits
static inline std::string check_items(const char* who, size_t n, uint64_t groups) {
    if ((uint64_t)n * groups > 0xffffffffull)
        return errorf("%s: %zu sets x %llu groups is too many items", who, n, (unsigned long long)groups);
    return std::string();
}

// ---- launch orders: the 8-register sets (wide[s] == 0) first, returning how many they are ---
// climb, census: the request's own order within each register file
static inline size_t request_order(const std::vector<uint8_t>& wide, const uint32_t* set_ids, size_t n,
                                   std::vector<uint32_t>& req) {
    req.clear();
    req.reserve(n);
    size_t n_narrow = 0;
    for (int part = 0; part < 2; ++part) {
        for (size_t i = 0; i < n; i++)
            if ((int)wide[set_ids[i]] == part) req.push_back(set_ids[i]);
        if (part == 0) n_narrow = req.size();
    }
    return n_narrow;
}

// stream: the batch's wave order (`order`: narrow first, longest first within each); tab is
// [the sets in launch order: n | each one's place in the request: n]
static inline size_t batch_order(const std::vector<uint32_t>& order, const std::vector<uint8_t>& wide,
                                 const uint32_t* set_ids, size_t n, std::vector<uint32_t>& tab) {
    std::vector<uint32_t> place(order.size(), 0xffffffffu);
    for (size_t i = 0; i < n; i++) place[set_ids[i]] = (uint32_t)i;
    tab.assign(2 * n, 0u);
    size_t k = 0, n_narrow = 0;
    for (uint32_t s : order) {
        if (place[s] == 0xffffffffu) continue;
        tab[k] = s;
        tab[n + k] = place[s];
        n_narrow += !wide[s];
        k++;
    }
    return n_narrow;
}

// ---- launch geometry -----------------------------------------------------------------------
// the knobs pathfeas.hip reads from the environment (read_env_knobs), at their defaults
struct Knobs {
    uint32_t waves_per_cu_full = 512;
    uint32_t waves_per_cu_early = 16;
    uint32_t early_chunk_groups = 8;
    uint32_t probe_max_sets = 64;
};

// one launch of persistent waves that take (set, slice) items from the queue heads
struct Grid {
    uint32_t per = 0, slices = 0;  // what an item covers (search: candidates, stream: groups); items per set
    uint64_t items = 0, waves = 0;
    uint32_t blocks = 0;
};

static inline uint32_t groups_of(uint32_t candidates) { return (uint32_t)(((uint64_t)candidates + 63u) / 64u); }

static inline void fill_grid(Grid& g, uint64_t n_sets, uint64_t slots) {
    g.items = n_sets * g.slices;
    g.waves = std::min<uint64_t>(g.items, slots);
    g.blocks = (uint32_t)((g.waves + PF_SEARCH_WG_WAVES - 1) / PF_SEARCH_WG_WAVES);
}

// One (phase, part) launch of a search over n_sets sets and `budget` candidates each: a
// chip-filling grid of persistent waves, in the full sweep as in the early-exit search, enough
// items to fill the CUs several times over, each covering >= 64 candidates of one set.
static inline Grid geometry(const Knobs& k, int num_cus, uint32_t n_sets, uint32_t budget, uint32_t flags) {
    const bool early = flags & PF_FLAG_EARLY_EXIT;
    const uint64_t groups = (budget + 63u) / 64u;  // 64-candidate groups per set
    uint64_t gpw;                                  // groups per item
    if (early) {
        // work-queue items: chunks of early_chunk_groups groups, larger when the batch
        // would make more than 64 items per wave — every item costs a claim (an L2 atomic,
        // ~14 ns per head) even when its set is already decided, which dominated planted
        // batches of 65,536 sets (tools/full_pass.py: 136 ms per 1M sets at 8 groups)
        const uint64_t max_items = (uint64_t)num_cus * k.waves_per_cu_early * 64u;
        gpw = std::max<uint64_t>(k.early_chunk_groups, (n_sets * groups + max_items - 1) / max_items);
        // small batches (the funnel's single queries, fork pairs): chunks small enough that
        // every wave slot of the grid gets an item, so a set without a witness among its
        // candidates takes one chunk's time per wave, not early_chunk_groups groups'
        const uint64_t slots = (uint64_t)num_cus * k.waves_per_cu_early;
        gpw = std::min(gpw, (n_sets * groups + slots - 1) / slots);
        gpw = std::max<uint64_t>(1, std::min<uint64_t>(gpw, groups));
    } else {
        const uint64_t target_waves = (uint64_t)num_cus * k.waves_per_cu_full;
        uint64_t sl = (target_waves + n_sets - 1) / std::max<uint32_t>(n_sets, 1u);
        sl = std::max<uint64_t>(1, std::min<uint64_t>(sl, groups));
        gpw = (groups + sl - 1) / sl;
    }
    Grid g;
    g.per = (uint32_t)(gpw * 64u);
    g.slices = std::max<uint32_t>(1u, (budget + g.per - 1) / g.per);
    fill_grid(g, n_sets, (uint64_t)num_cus * (early ? k.waves_per_cu_early : 16u));
    return g;
}

// Whether an early-exit search starts with the probe launch (candidates 0..63 of every set, one
// wave per set): 2 .. probe_max_sets sets that all carry a candidate 0, more than one group to
// search, and no PF_FLAG_NO_PROBE (pathfeas.hip has the measurements behind the rule).
static inline bool probe_first(const Knobs& k, size_t n_sets, uint32_t budget, uint32_t flags, bool all_parented) {
    return (flags & PF_FLAG_EARLY_EXIT) && budget > 64u && n_sets >= 2 && n_sets <= k.probe_max_sets && all_parented &&
           !(flags & PF_FLAG_NO_PROBE);
}

// climb, census: an item is one 64-candidate group of one set
static inline Grid group_grid(const Knobs& k, int num_cus, size_t n_sets, uint32_t groups) {
    Grid g;
    g.per = 1;
    g.slices = groups;
    fill_grid(g, n_sets, (uint64_t)num_cus * k.waves_per_cu_early);
    return g;
}

// work-queue items per wave slot that a stream launch aims for
constexpr uint64_t kStreamItemsPerWave = 32;

// stream: an item is a run of g.per groups of one set: about kStreamItemsPerWave items for every
// wave of a chip-filling grid (the claim and the set's descriptor are paid per item, the last
// item of a wave is the launch's tail), one group each while the grid is not full.  chunk_groups
// (PF_STREAM_CHUNK_GROUPS, 0: unset) overrides the run's length.
static inline Grid stream_grid(const Knobs& k, int num_cus, size_t n_sets, uint32_t groups, uint64_t chunk_groups) {
    const uint64_t slots = (uint64_t)num_cus * k.waves_per_cu_early;
    uint64_t per_item = std::max<uint64_t>(1, (uint64_t)n_sets * groups / (slots * kStreamItemsPerWave));
    if (chunk_groups) per_item = chunk_groups;
    per_item = std::min<uint64_t>(per_item, groups);
    Grid g;
    g.per = (uint32_t)per_item;
    g.slices = (uint32_t)((groups + per_item - 1) / per_item);
    fill_grid(g, n_sets, slots);
    return g;
}

// ---- counters ------------------------------------------------------------------------------
constexpr size_t kCounterBytes = PF_COUNTER_STRIPES * 128;  // the counter lines of a batch's scratch

// the PF_COUNTER_STRIPES lines of 16 words summed per slot: evals_full, cands_decided, ops,
// timed-out items and, after a stream call, the sets with a witness
static inline void sum_counters(const unsigned long long* hs, unsigned long long h[5]) {
    for (int k = 0; k < 5; k++) h[k] = 0;
    for (int i = 0; i < PF_COUNTER_STRIPES; i++)
        for (int k = 0; k < 5; k++) h[k] += hs[i * 16 + k];
}

}  // namespace pf_launch

#endif  // PF_LAUNCH_H
