// Host build of mythril_amd/csrc/pf_launch.h: the launch half of pathfeas.hip that makes no HIP
// call, stand-alone.
//   host_launch_check geometry FILE      every row of FILE (tests/host_launch_geometry.txt: what
//                                        the host driver computed before the rules moved into
//                                        the header) recomputed; prints "rows N", or the rows
//                                        that differ and exits 1
//   host_launch_check request WHO N_SETS MAX_ID none | null N | ID...
//                                        check_request's message, or "ok", for no ids, a null
//                                        set_ids of N entries, or the ids; a set above MAX_ID
//                                        fails the caller's own condition, "WHO: set ID is too
//                                        large" (MAX_ID "-": a caller without one)
//   host_launch_check order WIDE ORDER REQUEST    (comma-separated lists)
//                                        "request: <sets> n_narrow K" and
//                                        "batch: <sets> places <places> n_narrow K"
//   host_launch_check al                 al() of 0, 1, 255, 256, 257 and 2^32 + 1
//   host_launch_check counters           lines with 1000 * stripe + 10 * slot + 1 in slots 0..15:
//                                        the five sums
// stderr is left to the sanitizers tests/test_host_launch.py builds this with.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../mythril_amd/csrc/pf_launch.h"

using namespace pf_launch;

static std::vector<uint32_t> list_of(const char* s) {
    std::vector<uint32_t> v;
    for (const char* p = s; *p;) {
        char* end;
        v.push_back((uint32_t)strtoul(p, &end, 10));
        p = *end ? end + 1 : end;
    }
    return v;
}

static void print_list(const std::vector<uint32_t>& v, size_t from, size_t to) {
    for (size_t i = from; i < to; i++) printf(i == from ? "%u" : ",%u", v[i]);
}

static Knobs knobs_of(int which) {
    Knobs k;  // 0: the defaults
    if (which) {
        k.early_chunk_groups = 1;
        k.waves_per_cu_early = 8;
    }
    return k;
}

// One row of the table, recomputed: the row's inputs and then what the header gives for them,
// in the table's format.
static std::string recompute(const char* line) {
    char out[256] = "";
    int cus, early, allpar, noprobe, kn;
    uint32_t ns, budget, pmax;
    unsigned long long np, ov;
    if (sscanf(line, "C %d %" SCNu32 " %" SCNu32 " %d %d %d %" SCNu32 " %d", &cus, &ns, &budget, &early, &allpar,
               &noprobe, &pmax, &kn) == 8) {
        Knobs k = knobs_of(kn);
        k.probe_max_sets = pmax;
        const uint32_t flags = (early ? PF_FLAG_EARLY_EXIT : 0u) | (noprobe ? PF_FLAG_NO_PROBE : 0u);
        const bool probe = probe_first(k, ns, budget, flags, allpar != 0);
        // the search launch of an all-narrow batch: behind a probe it starts at candidate 64
        const Grid g = geometry(k, cus, ns, budget - (probe ? 64u : 0u), flags);
        snprintf(out, sizeof(out), "C %d %u %u %d %d %d %u %d %u %u %llu %llu %u %d", cus, ns, budget, early, allpar,
                 noprobe, pmax, kn, g.per, g.slices, (unsigned long long)g.items, (unsigned long long)g.waves,
                 g.blocks, (int)probe);
    } else if (sscanf(line, "P %d %" SCNu32 " %d", &cus, &ns, &kn) == 3) {
        const Grid g = geometry(knobs_of(kn), cus, ns, 64u, PF_FLAG_EARLY_EXIT);  // the probe: candidates 0..63
        snprintf(out, sizeof(out), "P %d %u %d %u %u %llu %llu %u", cus, ns, kn, g.per, g.slices,
                 (unsigned long long)g.items, (unsigned long long)g.waves, g.blocks);
    } else if (sscanf(line, "S %d %llu %" SCNu32 " %d %llu", &cus, &np, &budget, &kn, &ov) == 5) {
        const Grid g = stream_grid(knobs_of(kn), cus, (size_t)np, groups_of(budget), ov);
        const bool too_many = !check_items("stream", (size_t)np, groups_of(budget)).empty();
        snprintf(out, sizeof(out), "S %d %llu %u %d %llu %u %llu %llu %u %d", cus, np, budget, kn, ov, g.per,
                 (unsigned long long)g.items, (unsigned long long)g.waves, g.blocks, (int)too_many);
    } else if (sscanf(line, "K %d %llu %" SCNu32 " %d", &cus, &np, &budget, &kn) == 4) {
        const uint32_t groups = groups_of(budget);
        const Grid g = group_grid(knobs_of(kn), cus, (size_t)np, groups);
        const bool too_many = !check_items("climb", (size_t)np, groups).empty();
        snprintf(out, sizeof(out), "K %d %llu %u %d %u %llu %llu %u %d", cus, np, budget, kn, groups,
                 (unsigned long long)g.items, (unsigned long long)g.waves, g.blocks, (int)too_many);
    }
    return out;
}

static int geometry_rows(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) return 2;
    char line[256];
    size_t rows = 0, bad = 0;
    while (fgets(line, sizeof(line), f)) {
        line[strcspn(line, "\n")] = 0;
        if (line[0] == '#' || line[0] == 0) continue;
        rows++;
        const std::string got = recompute(line);
        if (got != line && bad++ < 20) printf("table: %s\nheader: %s\n", line, got.c_str());
    }
    fclose(f);
    printf("rows %zu\n", rows);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "geometry")) return geometry_rows(argv[2]);
    if (argc >= 6 && !strcmp(argv[1], "request")) {
        const char* who = argv[2];
        const size_t n_sets = strtoul(argv[3], nullptr, 10);
        const uint32_t max_id = (uint32_t)strtoul(argv[4], nullptr, 10);
        std::vector<uint32_t> ids(1, 0u);  // "none": a pointer to look at, and n == 0
        const bool null_ids = !strcmp(argv[5], "null"), none = !strcmp(argv[5], "none");
        if (null_ids && argc != 7) return 2;
        if (!null_ids && !none) ids.clear();
        for (int i = 5; !null_ids && !none && i < argc; i++) ids.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
        const uint32_t* p = null_ids ? nullptr : ids.data();
        const size_t n = null_ids ? strtoul(argv[6], nullptr, 10) : none ? 0 : ids.size();
        const std::string e = !strcmp(argv[4], "-") ? check_request(who, n_sets, p, n)
                                                    : check_request(who, n_sets, p, n, [&](uint32_t s) {
                                                          return s > max_id ? errorf("%s: set %u is too large", who, s)
                                                                            : std::string();
                                                      });
        printf("%s\n", e.empty() ? "ok" : e.c_str());
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "order")) {
        const std::vector<uint32_t> wide32 = list_of(argv[2]), order = list_of(argv[3]), req_in = list_of(argv[4]);
        const std::vector<uint8_t> wide(wide32.begin(), wide32.end());
        std::vector<uint32_t> req, tab;
        const size_t n = req_in.size();
        const size_t nn = request_order(wide, req_in.data(), n, req);
        printf("request: ");
        print_list(req, 0, req.size());
        printf(" n_narrow %zu\n", nn);
        const size_t nb = batch_order(order, wide, req_in.data(), n, tab);
        if (tab.size() != 2 * n) return 3;
        printf("batch: ");
        print_list(tab, 0, n);
        printf(" places ");
        print_list(tab, n, 2 * n);
        printf(" n_narrow %zu\n", nb);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "al")) {
        printf("%zu %zu %zu %zu %zu %zu\n", al(0), al(1), al(255), al(256), al(257), al(((size_t)1 << 32) + 1));
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "counters")) {
        static_assert(kCounterBytes == PF_COUNTER_STRIPES * 16 * sizeof(unsigned long long), "16 words per line");
        std::vector<unsigned long long> lines(kCounterBytes / 8);
        for (int i = 0; i < PF_COUNTER_STRIPES; i++)
            for (int k = 0; k < 16; k++) lines[i * 16 + k] = 1000ull * i + 10ull * k + 1;
        unsigned long long h[5];
        sum_counters(lines.data(), h);
        printf("%llu %llu %llu %llu %llu\n", h[0], h[1], h[2], h[3], h[4]);
        return 0;
    }
    return 2;
}
