// Host build of the site bookkeeping of mythril_amd/csrc/pf_devprog.h (device_sites, what
// pf_device_sites returns), stand-alone.
//   devsites_host_check IN OUT FOLD
// IN:  u64 n_ins, n_const, n_sets, then the u32 arrays code (4 per instruction), consts (8),
//      descs (8), as pf_device_sites takes them.
// OUT: u64 n_sites, n_sets, then u32 site_assert[n_sites] and u32 count[n_sets].
// FOLD is the PF_DEVICE_FOLD value (the PF_FOLD_MIN_SETS gate applies).  The program also checks
// the map against the device program the same passes give — one entry per site, in range — and
// prints what is wrong on stdout, exit 1; stderr is left to the sanitizers
// tests/test_devsites_host.py builds this with.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../mythril_amd/csrc/pf_devprog.h"

using namespace pf_devprog;

static std::vector<uint32_t> read_u32(FILE* f, size_t n) {
    std::vector<uint32_t> v(n);
    if (n && fread(v.data(), 4, n, f) != n) {
        printf("short input\n");
        exit(2);
    }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int fold = atoi(argv[3]);
    FILE* f = fopen(argv[1], "rb");
    uint64_t n[3];
    if (!f || fread(n, 8, 3, f) != 3) return 2;
    const size_t n_ins = n[0], n_const = n[1], n_sets = n[2];
    const std::vector<uint32_t> code = read_u32(f, 4 * n_ins), consts = read_u32(f, 8 * n_const),
                                dwords = read_u32(f, 8 * n_sets);
    fclose(f);
    static_assert(sizeof(pf_set_desc) == 32, "descs are 8 u32 each");
    std::vector<pf_set_desc> descs(n_sets);
    if (n_sets) memcpy(descs.data(), dwords.data(), 32 * n_sets);
    const uint32_t* pc = n_const ? consts.data() : nullptr;

    const SiteMap M = device_sites(code.data(), n_ins, pc, n_const, descs.data(), n_sets, fold);

    // the device program of the same passes, and its sites as the kernels count them (wave_order)
    const std::vector<uint32_t> fixed = stamped(code.data(), n_ins);
    std::vector<pf_set_desc> d = descs;
    std::vector<uint32_t> out, pool;
    device_program(fixed.data(), fixed.size(), d, prep_ranges(descs.data(), n_sets, n_ins), out, pc, n_const,
                   n_sets >= PF_FOLD_MIN_SETS ? fold : 0, &pool);
    const WaveOrder wo = wave_order(out.data(), d.data(), n_sets, std::vector<uint8_t>(n_sets, 0));
    if (M.cnt.size() != n_sets) {
        printf("%zu counts for %zu sets\n", M.cnt.size(), n_sets);
        return 1;
    }
    size_t off = 0;
    for (size_t s = 0; s < n_sets; s++) {
        if (M.cnt[s] != wo.sites[s]) {
            printf("set %zu: %u sites mapped, %u in the device program\n", s, M.cnt[s], wo.sites[s]);
            return 1;
        }
        uint32_t n_assert = 0;
        for (uint32_t i = 0; i < descs[s].n_ins; i++)
            n_assert += pf_ins_op(code[4 * ((size_t)descs[s].code_off + i)]) == PF_ASSERT;
        for (uint32_t j = 0; j < M.cnt[s]; j++) {
            if (off + j >= M.asserts.size() || M.asserts[off + j] >= n_assert) {
                printf("set %zu site %u: assert ordinal out of range (%u asserts)\n", s, j, n_assert);
                return 1;
            }
        }
        off += M.cnt[s];
    }
    if (off != M.asserts.size()) {
        printf("%zu entries for %zu sites\n", M.asserts.size(), off);
        return 1;
    }
    const uint64_t m[2] = {M.asserts.size(), n_sets};
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(m, 8, 2, o);
    if (!M.asserts.empty()) fwrite(M.asserts.data(), 4, M.asserts.size(), o);
    if (n_sets) fwrite(M.cnt.data(), 4, n_sets, o);
    return fclose(o) ? 2 : 0;
}
