// Host build of mythril_amd/csrc/pf_devprog.h: the validator and the preparation of a packed
// batch, stand-alone.
//   devprog_host_check IN OUT FOLD own|single batch|program
// IN:  u64 n_ins, n_const, n_vars, n_parents, n_sets, then the u32 arrays code (4 per
//      instruction), consts (8), schema (4), descs (8), as pf_batch_create takes them.
// OUT: u64 n_ins, n_sets, n_const of the result, then its u32 arrays code, descs, pool.
// FOLD is the PF_DEVICE_FOLD value.  "batch" is what pf_batch_create uploads (and
// pf_device_batch returns): every set validated, the PF_FOLD_MIN_SETS gate, the device pool.
// "program" is pf_device_program: no validation, no gate, the caller's pool.  "own" takes the
// driver's set ranges (prepare_program and its host threads for a batch), "single" the one
// range {0, n_sets}; stdout says "ranges N", how many ranges that was.  A rejected batch prints
// the validator's message on stdout and exits 1; stderr is left to the sanitizers
// tests/test_devprog_host.py builds this with.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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
    if (argc != 6) return 2;
    const int fold = atoi(argv[3]);
    const bool single = !strcmp(argv[4], "single"), batch = !strcmp(argv[5], "batch");
    FILE* f = fopen(argv[1], "rb");
    uint64_t n[5];
    if (!f || fread(n, 8, 5, f) != 5) return 2;
    const size_t n_ins = n[0], n_const = n[1], n_vars = n[2], n_parents = n[3], n_sets = n[4];
    const std::vector<uint32_t> code = read_u32(f, 4 * n_ins), consts = read_u32(f, 8 * n_const),
                                schema = read_u32(f, 4 * n_vars), dwords = read_u32(f, 8 * n_sets);
    fclose(f);
    static_assert(sizeof(pf_set_desc) == 32, "descs are 8 u32 each");
    std::vector<pf_set_desc> descs(n_sets);
    if (n_sets) memcpy(descs.data(), dwords.data(), 32 * n_sets);
    const uint32_t* pc = n_const ? consts.data() : nullptr;

    Prepared R;
    if (batch && !single) {
        R = prepare_program(code.data(), n_ins, pc, n_const, schema.data(), n_vars, n_parents, descs.data(), n_sets,
                            fold);
    } else {
        std::vector<uint32_t> fixed = batch ? std::vector<uint32_t>(4 * n_ins) : stamped(code.data(), n_ins);
        R.wide.assign(n_sets, 0);
        for (size_t s = 0; batch && s < n_sets && R.err.empty(); s++)
            R.err = check_set(s, code.data(), n_ins, n_const, schema.data(), n_vars, n_parents, descs.data(),
                              fixed.data(), R.wide.data());
        if (R.err.empty()) {
            R.descs = descs;
            const std::vector<size_t> cut =
                single ? std::vector<size_t>{0, n_sets} : prep_ranges(descs.data(), n_sets, n_ins);
            device_program(fixed.data(), fixed.size(), R.descs, cut, R.code, pc, n_const,
                           !batch || n_sets >= PF_FOLD_MIN_SETS ? fold : 0, batch ? &R.pool : nullptr);
        }
    }
    if (!R.err.empty()) {
        printf("%s\n", R.err.c_str());
        return 1;
    }
    printf("ranges %zu\n", single ? (size_t)1 : prep_ranges(descs.data(), n_sets, n_ins).size() - 1);
    const std::vector<uint32_t>& pool = R.pool.empty() ? consts : R.pool;
    const uint64_t m[3] = {R.code.size() / 4, n_sets, pool.size() / 8};
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(m, 8, 3, o);
    if (!R.code.empty()) fwrite(R.code.data(), 4, R.code.size(), o);
    if (n_sets) fwrite(R.descs.data(), 32, n_sets, o);
    if (!pool.empty()) fwrite(pool.data(), 4, pool.size(), o);
    return fclose(o) ? 2 : 0;
}
