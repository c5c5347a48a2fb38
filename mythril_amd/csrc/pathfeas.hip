// pathfeas.hip — host side of libpathfeas.so: the C ABI declared in include/pathfeas.h.
//
// Single translation unit: the kernels (pf_eval.hip, pf_keccak.hip) are included so the
// launches need no relocatable device code.  All entry points serialise on one mutex and
// re-select the device, because Mythril's query funnel calls in from a new worker thread
// per query (mythril/support/model.py:99-117).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pathfeas.h"
#include "pf_devprog.h"
#include "pf_launch.h"
#include "pf_eval.hip"
#include "pf_keccak.hip"

namespace {

// the host half — validator, device-program rewrites, threaded preparation, wave order
using namespace pf_devprog;
// request checks, launch orders, launch geometry, the counter sum, al()
using namespace pf_launch;

std::mutex g_mu;
thread_local std::string g_err_tls;
std::string g_err;
// g_err is written under g_mu only.  Work done without the lock (pf_devprog.h's preparation,
// pf_batch_create's device lookup and upload) returns its error as a string, which its caller
// moves into g_err under the lock (set_err).
int set_err(const std::string& e) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_err = e;
    return -1;
}

// One entry per initialised device (pf_init's mask): its library stream, timing events for
// the Keccak launches and the launch geometry inputs.  Batches live on one device each and
// carry their own counters and events, so launches of different batches never share scratch.
struct Dev {
    int id = -1;            // the HIP device
    int key = -1;           // what the API calls it: the device id (pf_init) or a context id
                            // >= PF_CONTEXT_BASE (pf_init_contexts: several per device)
    hipStream_t stream = nullptr;
    hipStream_t up_stream = nullptr;  // batch uploads, issued outside g_mu (pf_batch_create)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int num_cus = 256;
    hipStream_t last_stream = nullptr;  // see switch_stream
    // device blocks of freed batches, reused by later batches that fit: a query's batch is
    // created and freed per call, and hipMalloc + hipFree (which synchronises the device)
    // per buffer were a millisecond of the single-query latency
    std::vector<std::pair<void*, size_t>> pool;
    // timing events of freed batches, reused (hipEventCreate / Destroy per batch were two
    // runtime calls each on the single-query path); under g_pool_mu
    std::vector<hipEvent_t> ev_free;
};
// ascending keys.  The entries are heap objects that stay put until pf_shutdown, so a Dev*
// taken by pf_batch_create (which runs without g_mu) survives a concurrent pf_init /
// pf_init_contexts growing and re-sorting the vector; the vector itself is read and changed
// under g_devs_mu (and changed only while g_mu is held too, so readers under g_mu need no more).
std::vector<std::unique_ptr<Dev>> g_devs;
std::mutex g_devs_mu;
int g_default = -1;       // index in g_devs of the default device (lowest id)
// search-kernel waves launched per CU (PF_WAVES_PER_CU overrides both).  Measured on config 3
// (1024 sets x 65,536 candidates, profiles/r01_wavesweep.md): with the longest-first set order
// the full sweep peaks at 512 (finer slices even out the sets' unequal costs in the last round
// of waves; 64 was 17 % slower).  The early-exit search is a work queue of (set, chunk) items
// taken by a chip-filling grid: 16 waves per CU (4 per SIMD, the narrow kernels' occupancy;
// PF_WAVES_PER_CU_EARLY), chunks of early_chunk_groups 64-candidate groups
// (PF_EARLY_CHUNK_GROUPS).
// Early-exit searches of 2 .. probe_max_sets sets that all carry a parent / hint model
// (candidate 0) start with a probe launch: one wave per set evaluates only candidates 0..63,
// then the queue search runs behind it on the stream from candidate 64 and skips every set the
// probe decided.  Without it every wave of the chip-filling grid claims its item before any
// witness exists, so the grid evaluates one group per wave at 4 waves/SIMD and the candidate-0
// waves finish at that contention.  Measured (tools/search_overhead_probe.py,
// profiles/r04o_search_overhead_probe.log, after the striped counters made a grid of skipping
// waves cheap): 4 planted sets 0.130 -> 0.110 ms, 16: 0.175 -> 0.128 ms; one set 0.064 ->
// 0.071 ms and sets without a candidate-0 witness (16 unplanted: 0.237 -> 0.321 ms) lose, hence
// the conditions.  (Round 4 before the striped counters: a single funnel query 0.686 -> 0.770 ms
// with the probe on for every batch.)  PF_PROBE_MAX_SETS sets the bound, 0 turns it off.
// A set without variables counts as parented (all its candidates are candidate 0), and the
// caller's PF_FLAG_NO_PROBE skips the probe when it knows a set's candidate 0 misses (check_sets:
// a host hint model that leaves a root false — the probe of a long program then only delays
// the search behind it; profiles/r06_probe_rule.md).
// pf_launch.h has the defaults and the rules (geometry, probe_first), which take the knobs as an
// argument; read_env_knobs overrides them.
Knobs g_knobs;
// PF_DEVICE_FOLD as read at init (pf_devprog.h device_fold_env): what pf_batch_create folds with
int g_device_fold = 1;

int fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return -1;
}

// the header's checks return their message: empty is no error
bool failed(const std::string& e) {
    if (!e.empty()) g_err = e;
    return !e.empty();
}

#define HIPCHK(x)                                                                       \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), \
                                          __FILE__, __LINE__);                          \
    } while (0)
// inside a pooled round trip (Pooled): the entry point's own message
#define HIPTRY(who, x)                                                  \
    do {                                                                \
        if ((x) != hipSuccess) return fail("%s: HIP call failed", who); \
    } while (0)

// A batch's device blocks.  The main block holds the arrays pf_batch_create uploads; each of the
// others is acquired by the batch's first call of its entry point (ensure) and lives as long as
// the batch.
enum Side { kMain, kClimb, kCensus, kStream, kLink, kSides };
struct Block { void* mem = nullptr; size_t cap = 0; };

struct Batch {
    int device;
    Block side[kSides];
    size_t n_vars, n_sets;
    uint32_t max_vars;
    size_t n_narrow = 0;    // d_order[0, n_narrow): sets whose programs write only W registers
                            // < PF_NW_NARROW (8-register kernels, 3 waves/SIMD); the rest run
                            // the 16-register kernels in a second launch
    std::vector<pf_set_desc> h_descs;
    pf_set_desc* d_descs = nullptr;
    uint4* d_code = nullptr;
    uint32_t* d_consts = nullptr;
    uint4* d_schema = nullptr;
    uint32_t* d_parents = nullptr;
    uint32_t* d_found = nullptr;
    uint32_t* d_order = nullptr;    // set ids, most expensive first (search-kernel wave order)
    bool all_parented = false;      // every set carries a parent / hint model (candidate 0) or
                                    // has no variables
    uint32_t* d_scratch = nullptr;  // this batch's t0 (u64 [4]), queue heads and counter lines (pf_bytecode.h)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // climb (pf_climb_batch): per set, whether it runs the 16-register kernels and the assert
    // sites of its device program; the climb block holds working descriptors and schema (every
    // variable parented), the two parent buffers and the per-set states
    std::vector<uint8_t> h_wide;
    std::vector<uint32_t> h_sites;
    // census (pf_census_batch): the census block holds per-set states, the rows holds / alive /
    // sole of every set and this call's tables
    // stream (pf_eval_batch): d_order's host copy, and the stream block — a call's sets in launch
    // order and their places in the request, n_sets u32 each; e_req is what the block holds (a
    // call with the same request uploads nothing)
    std::vector<uint32_t> h_order;
    std::vector<uint32_t> e_req;
    // linked search (pf_check_linked): host copies of what a link group's members share, and
    // the link block — this call's group of every set and members of every group, the groups'
    // verdicts, one (mask, count) record per group and 64 candidates — the one block whose size
    // depends on the call: grown when a later call needs more; l_req is the group_of it holds
    LinkTables h_link;
    std::vector<uint32_t> l_req;

    // views of the scratch (pf_bytecode.h).  The kernels take the scratch's base for their
    // counters and add PF_COUNTER_OFF themselves.
    static constexpr size_t kT0Word = 8;  // t0 starts 32 bytes in
    unsigned long long* counters() const { return reinterpret_cast<unsigned long long*>(d_scratch); }
    uint64_t* t0() const { return reinterpret_cast<uint64_t*>(d_scratch + kT0Word); }
    // the work-queue heads of one (phase, part) launch; climb, census and stream have one phase
    uint32_t* queue(int phase, int part) const {
        return d_scratch + PF_EARLY_QUEUE_OFF / 4 + (phase * 2 + part) * PF_EARLY_QUEUES * PF_EARLY_QUEUE_STRIDE;
    }
    const uint32_t* counter_lines() const { return d_scratch + PF_COUNTER_OFF / 4; }

    ~Batch() {  // the device blocks go back to their device's pool first (release_batch)
        for (Block& b : side)
            if (b.mem) hipFree(b.mem);
        if (ev0) hipEventDestroy(ev0);
        if (ev1) hipEventDestroy(ev1);
    }
};

Dev* find_dev(int key) {
    for (auto& d : g_devs)
        if (d->key == key) return d.get();
    return nullptr;
}

constexpr size_t kPoolBlocks = 8;
// the device pools have their own lock: pf_batch_create takes and returns blocks without
// g_mu (a search holds g_mu until its results are back)
std::mutex g_pool_mu;

// a device block of at least `bytes` from the device's pool (smallest that fits and wastes
// at most 4x), else a new one
void* pool_acquire(Dev* D, size_t bytes, size_t* cap) {
    std::lock_guard<std::mutex> pk(g_pool_mu);
    size_t best = SIZE_MAX;
    for (size_t i = 0; i < D->pool.size(); ++i)
        if (D->pool[i].second >= bytes && D->pool[i].second <= 4 * bytes + (1u << 20) &&
            (best == SIZE_MAX || D->pool[i].second < D->pool[best].second))
            best = i;
    if (best != SIZE_MAX) {
        void* p = D->pool[best].first;
        *cap = D->pool[best].second;
        D->pool.erase(D->pool.begin() + best);
        return p;
    }
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    *cap = bytes;
    return p;
}

// a block back into its device's pool (the oldest block is released when the pool is full).
// Nothing that uses the block may be in flight.
void pool_release(Dev* D, void* p, size_t cap) {
    std::lock_guard<std::mutex> pk(g_pool_mu);
    if (D->pool.size() >= kPoolBlocks) {
        hipFree(D->pool.front().first);
        D->pool.erase(D->pool.begin());
    }
    D->pool.emplace_back(p, cap);
}

// A block that work still in flight may read or write (a copy or a synchronisation failed) is
// not pooled again: it is freed after a full device synchronisation, whose own failure leaks it
// rather than hand memory in use to the next pool_acquire.
void free_in_flight(void* p) {
    if (hipDeviceSynchronize() == hipSuccess) hipFree(p);
}

// One pooled block for a call's round trip: copy in, launch, copy out, stream synchronised.
// release() hands it back to the pool once the stream is drained; a return before that (a failed
// HIP call) leaves it to free_in_flight.
struct Pooled {
    Dev* D;
    uint8_t* p = nullptr;
    size_t cap = 0;
    // in the body: pool_acquire writes cap, which a member initialiser would then reset
    Pooled(Dev* D, size_t bytes) : D(D) { p = static_cast<uint8_t*>(pool_acquire(D, bytes, &cap)); }
    Pooled(const Pooled&) = delete;
    void release() {
        pool_release(D, p, cap);
        p = nullptr;
    }
    ~Pooled() {
        if (p) free_in_flight(p);
    }
};

// B's side block `kind` with room for `bytes`: acquired by the first call that needs it,
// replaced when a call needs more (nothing of the batch is in flight: every earlier call on it
// returned after its results).  *fresh: the block is new, whatever the caller remembers of its
// contents is gone.
int ensure(Dev* D, Batch* B, Side kind, size_t bytes, const char* who, bool* fresh = nullptr) {
    Block& b = B->side[kind];
    if (fresh) *fresh = !b.mem || b.cap < bytes;
    if (b.mem && b.cap < bytes) {
        pool_release(D, b.mem, b.cap);
        b.mem = nullptr;
    }
    if (!b.mem) {
        b.mem = pool_acquire(D, bytes, &b.cap);
        if (!b.mem) return fail("%s: hipMalloc(%zu) failed", who, bytes);
    }
    return 0;
}

// free a batch: its blocks are kept for reuse.  Called with no launch of the batch in flight
// (pf_batch_free drains the stream of the device's last launch).
void release_batch(Dev* D, Batch* B) {
    for (Block& b : B->side) {
        if (!D || !b.mem) continue;
        pool_release(D, b.mem, b.cap);
        b.mem = nullptr;
    }
    if (D) {
        std::lock_guard<std::mutex> pk(g_pool_mu);
        for (hipEvent_t* e : {&B->ev0, &B->ev1}) {
            if (*e && D->ev_free.size() < 64) {
                D->ev_free.push_back(*e);
                *e = nullptr;
            }
        }
    }
    delete B;
}

// an event from the device's free list, else a new one
hipError_t event_acquire(Dev* D, hipEvent_t* e) {
    {
        std::lock_guard<std::mutex> pk(g_pool_mu);
        if (!D->ev_free.empty()) {
            *e = D->ev_free.back();
            D->ev_free.pop_back();
            return hipSuccess;
        }
    }
    return hipEventCreate(e);
}

// A launch on a caller's stream (the *_dev entry points) returns without waiting; before the
// device's next launch on a different stream reuses the Keccak events or a batch it reads,
// that stream is drained.
int switch_stream(Dev* D, hipStream_t st) {
    if (D->last_stream && D->last_stream != st) HIPCHK(hipStreamSynchronize(D->last_stream));
    D->last_stream = st;
    return 0;
}

// select (and make current) a device: the default one for device < 0.  An error goes to g_err,
// or to *err for the one caller that does not hold g_mu (pf_batch_create_on)
Dev* use_dev(int device, std::string* err = nullptr) {
    std::string e;
    Dev* D = g_devs.empty() ? nullptr : device < 0 ? g_devs[g_default].get() : find_dev(device);
    if (g_devs.empty()) e = "pf_init() has not been called";
    else if (!D) e = errorf("device %d was not initialised by pf_init", device);
    else if (hipError_t h = hipSetDevice(D->id)) e = errorf("hipSetDevice(%d): %s", D->id, hipGetErrorString(h));
    if (e.empty()) return D;
    (err ? *err : g_err) = e;
    return nullptr;
}

Batch* as_batch(uint64_t h) { return reinterpret_cast<Batch*>(static_cast<uintptr_t>(h)); }

hipStream_t pick_stream(Dev* D, void* s) { return s ? reinterpret_cast<hipStream_t>(s) : D->stream; }

// the search kernels by [early exit][16-register part]; the linked ones take the link block
// where the others take found[]
decltype(&pf_check_kernel) const kCheckKernels[2][2] = {{pf_check_kernel, pf_check_r16_kernel},
                                                         {pf_check_early_kernel, pf_check_early_r16_kernel}};
decltype(&pf_check_linked_kernel) const kLinkedKernels[2][2] = {
    {pf_check_linked_kernel, pf_check_linked_r16_kernel},
    {pf_check_linked_early_kernel, pf_check_linked_early_r16_kernel}};

// What every launch sequence on a batch starts with: t0 and the profiling slots at the scratch's
// front, the work-queue heads of every launch from PF_EARLY_QUEUE_OFF, the counter lines from
// PF_COUNTER_OFF and the first nf words of found[] in one fill, then B's first event.
int reset_scratch(Batch* B, hipStream_t st, uint32_t* d_found, uint32_t nf) {
    const uint32_t nz = PF_SCRATCH_BYTES / 4;
    const uint32_t blocks = std::min<uint32_t>((nz + nf + 255u) / 256u, 1024u);
    hipLaunchKernelGGL(pf_reset_kernel, dim3(blocks), dim3(256), 0, st, B->d_scratch, nz, d_found, nf);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(B->ev0, st));
    return 0;
}

// Enqueue one search over batch B on stream st (B's device must be current).  With `link` it is
// the linked search: the same phases, parts and geometry, the pf_check_linked_* kernels, the
// link block reset in found[]'s place (d_found is then not touched).
int check_enqueue(Batch* B, uint64_t gseed, uint32_t budget, uint32_t flags, uint32_t timeout_ms,
                  uint32_t* d_found, hipStream_t st, const LinkArgs* link = nullptr, uint32_t n_link_groups = 0) {
    Dev* D = find_dev(B->device);
    if (reset_scratch(B, st, d_found, link ? 0u : (uint32_t)std::max<size_t>(B->n_sets, 1))) return -1;
    if (link) {
        const uint64_t n_rec = (uint64_t)n_link_groups * link->words;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_rec + n_link_groups + 255u) / 256u, 1024u);
        hipLaunchKernelGGL(pf_link_init_kernel, dim3(blocks), dim3(256), 0, st, link->found, n_link_groups, link->mask,
                           link->count, n_rec);
        HIPCHK(hipGetLastError());
    }
    const uint64_t deadline = timeout_ms ? (uint64_t)timeout_ms * 100000ull : 0ull;  // 100 MHz
    const bool early = flags & PF_FLAG_EARLY_EXIT;
    // phase 0: the probe (early exit, small batches: candidates 0..63 of every set, one wave
    // per set); phase 1: the search over the whole budget, whose waves skip decided sets
    const bool probe = probe_first(g_knobs, B->n_sets, budget, flags, B->all_parented);
    for (int phase = probe ? 0 : 1; phase < 2; ++phase) {
        const uint32_t pbudget = phase == 0 ? 64u : budget;
        // the 8-register sets first, then the 16-register ones (usually none)
        for (int part = 0; part < 2; ++part) {
            const size_t first = part ? B->n_narrow : 0;
            const size_t n = part ? B->n_sets - B->n_narrow : B->n_narrow;
            if (n == 0 || budget == 0) continue;
            // phase 1 after a probe: candidates 64.. only (the probe evaluated 0..63)
            const uint32_t cbegin = (phase == 1 && probe) ? 64u : 0u;
            // a chip-filling grid of persistent waves takes the items from this launch's queue
            // heads (each (phase, part) launch has its own, all zeroed by the reset above)
            const Grid g = geometry(g_knobs, D->num_cus, (uint32_t)n, pbudget - cbegin, flags);
            if (g.items > 0xffffffffull) return fail("batch too large: %llu waves", (unsigned long long)g.items);
            auto launch = [&](auto kernel, auto verdicts) {
                hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(64 * PF_SEARCH_WG_WAVES), 0, st, B->d_descs,
                                   B->d_order + first, (uint32_t)n, B->d_code, B->d_consts, B->d_schema, B->d_parents,
                                   gseed, pbudget, g.per, g.slices, flags, deadline, B->t0(), verdicts, B->counters(),
                                   B->queue(phase, part), cbegin);
            };
            if (link) launch(kLinkedKernels[early][part], *link);
            else launch(kCheckKernels[early][part], d_found);
            HIPCHK(hipGetLastError());
        }
    }
    HIPCHK(hipEventRecord(B->ev1, st));
    return 0;
}

// Pinned host staging for the counter lines and verdicts a search reads back: a copy into
// pageable memory is staged and synchronous in the runtime (two of them were ~25 us of a
// single-query search's ~45 us outside the kernel); one buffer for the process (every entry
// point that reads results back holds g_mu), grown on demand, never shrunk, kept to process
// exit.  nullptr (pageable fallback) if the allocation fails.
uint8_t* pinned_staging(size_t bytes) {
    struct Pin {
        uint8_t* p = nullptr;
        size_t cap = 0;
    };
    static Pin t;
    if (bytes > t.cap) {
        if (t.p) (void)hipHostFree(t.p);
        t.p = nullptr;
        t.cap = 0;
        const size_t cap = std::max<size_t>((bytes + 65535) & ~size_t(65535), 65536);
        void* p = nullptr;
        if (hipHostMalloc(&p, cap, hipHostMallocPortable) != hipSuccess) return nullptr;
        t.p = static_cast<uint8_t*>(p);
        t.cap = cap;
    }
    return t.p;
}

// Pinned host staging for batch uploads (pf_batch_create), separate from pinned_staging and
// guarded by its own lock: an upload fills and copies it without holding g_mu.
std::mutex g_up_mu;
uint8_t* upload_staging(size_t bytes) {
    static uint8_t* p = nullptr;
    static size_t cap = 0;
    if (bytes > cap) {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const size_t c = std::max<size_t>((bytes + (1u << 20) - 1) & ~size_t((1u << 20) - 1), 1u << 20);
        void* q = nullptr;
        if (hipHostMalloc(&q, c, hipHostMallocPortable) != hipSuccess) return nullptr;
        p = static_cast<uint8_t*>(q);
        cap = c;
    }
    return p;
}

// What the launches between B's events left, from the counter lines as read back (the caller
// copies them with its own results and synchronises once): the lines summed, the events' time.
// The entry points differ in what their kernels count:
enum StatsOf {
    kSearchStats,  // n_sat is the caller's; ops and timeouts are counted
    kSideStats,    // climb, census: the same without ops
    kStreamStats   // n_sat is the lines' slot 4 (the sets with a witness), no ops, no timeouts
};
int fill_stats(Batch* B, const unsigned long long* lines, StatsOf of, uint64_t n_sat, pf_stats* stats) {
    unsigned long long h[5];
    sum_counters(lines, h);
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, B->ev0, B->ev1));
    stats->evals_full = h[0];
    stats->cands_decided = h[1];
    stats->ops = of == kSearchStats ? h[2] : 0;
    stats->n_sat = of == kStreamStats ? h[4] : n_sat;
    stats->kernel_ms = ms;
    stats->timed_out = of != kStreamStats && h[3] ? 1u : 0u;
    return 0;
}

// Wait for B's last search or stream call on stream st and read its counters and kernel time;
// with `found`, the verdicts too, copied before the one stream synchronisation (a second round
// trip was ~4 % of a single query's search).  A search's n_sat is left 0 for the caller
// (found_to_host).
// (d_from, n_from): the verdicts' device buffer and count when they are not the batch's found[]
// (the linked search's group verdicts)
int check_collect(Batch* B, hipStream_t st, StatsOf of, pf_stats* stats, std::vector<uint32_t>* found = nullptr,
                  const uint32_t* d_from = nullptr, size_t n_from = 0) {
    const size_t nf = d_from ? n_from : std::max<size_t>(B->n_sets, 1);
    if (!d_from) d_from = B->d_found;
    unsigned long long hs[kCounterBytes / 8];
    uint8_t* pin = pinned_staging(kCounterBytes + (found ? nf * 4 : 0));
    const uint32_t* d_lines = B->counter_lines();
    if (found) found->assign(nf, 0u);
    if (found && pin && d_from == d_lines + kCounterBytes / 4) {
        // the batch block keeps found[] right after the counter lines: one copy (each copy is
        // a blit dispatch serialised behind the search)
        HIPCHK(hipMemcpyAsync(pin, d_lines, kCounterBytes + nf * 4, hipMemcpyDeviceToHost, st));
    } else {
        HIPCHK(hipMemcpyAsync(pin ? static_cast<void*>(pin) : static_cast<void*>(hs), d_lines, kCounterBytes,
                              hipMemcpyDeviceToHost, st));
        if (found)
            HIPCHK(hipMemcpyAsync(pin ? static_cast<void*>(pin + kCounterBytes) : static_cast<void*>(found->data()),
                                  d_from, nf * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    if (pin) {
        memcpy(hs, pin, kCounterBytes);
        if (found) memcpy(found->data(), pin + kCounterBytes, nf * 4);
    }
    pf_stats unused;
    return fill_stats(B, hs, of, 0, stats ? stats : &unused);
}

// The two copies of a pooled round trip.  With the pinned staging buffer (pin) each is one copy
// through it: no pageable copies, which are staged and synchronous in the runtime.  Without
// (pin null: its allocation failed) they go straight from and to the caller's memory.
struct Piece { size_t off; const void* src; size_t bytes; };  // off: in the block and in the staging buffer
// in: the pieces to dm + off — staged, one copy of [0, the last piece's end)
hipError_t copy_in(uint8_t* dm, uint8_t* pin, std::initializer_list<Piece> pieces, hipStream_t st) {
    size_t end = 0;
    for (const Piece& c : pieces) {
        end = c.off + c.bytes;
        if (!c.bytes) continue;
        if (pin) memcpy(pin + c.off, c.src, c.bytes);
        else if (hipError_t e = hipMemcpyAsync(dm + c.off, c.src, c.bytes, hipMemcpyHostToDevice, st)) return e;
    }
    return pin ? hipMemcpyAsync(dm, pin, end, hipMemcpyHostToDevice, st) : hipSuccess;
}
// out: `bytes` at d to `out`, and the stream drained.  The staging buffer is reused: the stream
// orders this copy after the launch, which has consumed the copy-in.
hipError_t copy_out(void* out, const uint8_t* d, size_t bytes, uint8_t* pin, hipStream_t st) {
    if (hipError_t e = hipMemcpyAsync(pin ? static_cast<void*>(pin) : out, d, bytes, hipMemcpyDeviceToHost, st)) return e;
    if (hipError_t e = hipStreamSynchronize(st)) return e;
    if (pin) memcpy(out, pin, bytes);
    return hipSuccess;
}

}  // namespace

extern "C" {

int pf_version(void) { return 4; }

// Host only (no HIP call, tests/test_device_program.py): the program pf_batch_create would put
// on the device — traffic / unit bits recomputed from the opcodes, then the fold pass (whatever
// the batch's size: pf_batch_create skips it below PF_FOLD_MIN_SETS sets) and the peepholes.
// code_out needs room for n_ins instructions (the peepholes only delete); descs_out n_sets.
int pf_device_program(const uint32_t* code, size_t n_ins, const uint32_t* consts, size_t n_const,
                      const pf_set_desc* descs, size_t n_sets, uint32_t* code_out, size_t* n_ins_out,
                      pf_set_desc* descs_out) {
    const std::vector<uint32_t> fixed = stamped(code, n_ins);
    std::vector<pf_set_desc> d(descs, descs + n_sets);
    std::vector<uint32_t> out;
    device_program(fixed.data(), fixed.size(), d, prep_ranges(descs, n_sets, n_ins), out, consts, n_const,
                   device_fold_env());
    memcpy(code_out, out.data(), out.size() * 4);
    *n_ins_out = out.size() / 4;
    memcpy(descs_out, d.data(), n_sets * sizeof(pf_set_desc));
    return 0;
}

// Host only: what pf_batch_create uploads for this batch — the device programs, the device
// constant pool they index (device_program: the caller's constants, then the sets' own) and
// the descriptors with code_off and const_off re-based.  Unlike pf_device_program it applies
// pf_batch_create's PF_FOLD_MIN_SETS gate, and its code is readable only against consts_out.
// PF_DEVICE_FOLD is read on every call.  consts_out has room for consts_cap constants;
// *n_const_out is the pool's size, and a smaller consts_cap fails with nothing written.
int pf_device_batch(const uint32_t* code, size_t n_ins, const uint32_t* consts, size_t n_const,
                    const pf_set_desc* descs, size_t n_sets, uint32_t* code_out, size_t* n_ins_out,
                    pf_set_desc* descs_out, uint32_t* consts_out, size_t consts_cap, size_t* n_const_out) {
    const std::vector<uint32_t> fixed = stamped(code, n_ins);
    std::vector<pf_set_desc> d(descs, descs + n_sets);
    std::vector<uint32_t> out, pool;
    device_program(fixed.data(), fixed.size(), d, prep_ranges(descs, n_sets, n_ins), out, consts, n_const,
                   n_sets >= PF_FOLD_MIN_SETS ? device_fold_env() : 0, &pool);
    const uint32_t* pc = pool.empty() ? consts : pool.data();
    const size_t np = pool.empty() ? n_const : pool.size() / 8;
    *n_const_out = np;
    if (np > consts_cap)
        return set_err(errorf("pf_device_batch: the device pool holds %zu constants, room for %zu", np, consts_cap));
    memcpy(code_out, out.data(), out.size() * 4);
    *n_ins_out = out.size() / 4;
    memcpy(descs_out, d.data(), n_sets * sizeof(pf_set_desc));
    if (np && pc) memcpy(consts_out, pc, np * 32);
    return 0;
}

// Host only: the PF_ASSERT of the lowered program behind every assert site of the device programs
// pf_batch_create would upload for this batch (pf_devprog.h device_sites: pf_device_batch's gate,
// PF_DEVICE_FOLD read on every call).
int pf_device_sites(const uint32_t* code, size_t n_ins, const uint32_t* consts, size_t n_const,
                    const pf_set_desc* descs, size_t n_sets, uint32_t* site_assert_out, uint32_t* n_out) {
    const SiteMap M = device_sites(code, n_ins, consts, n_const, descs, n_sets, device_fold_env());
    if (M.asserts.size() > n_ins || M.cnt.size() != n_sets)
        return set_err(errorf("pf_device_sites: %zu sites of %zu sets for %zu instructions", M.asserts.size(),
                              M.cnt.size(), n_ins));
    if (!M.asserts.empty()) memcpy(site_assert_out, M.asserts.data(), M.asserts.size() * 4);
    if (n_sets) memcpy(n_out, M.cnt.data(), n_sets * 4);
    return 0;
}

#ifdef PF_PROFILE_UNITS
// profiling builds only (tools/unitprof.py): per-unit s_memtime cycles of a batch's last launch
int pf_prof_read(uint64_t handle, uint64_t* out) {
    std::lock_guard<std::mutex> lk(g_mu);
    Batch* B = as_batch(handle);
    if (!B || !use_dev(B->device)) return -1;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, B->d_scratch + 2 * PF_PROF_SLOT, (PF_PROF_BUCKETS + 1) * 8,
                     hipMemcpyDeviceToHost));
    return 0;
}
#endif

const char* pf_last_error(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_err_tls = g_err;
    return g_err_tls.c_str();
}

int pf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// The host lowering (libpflower.so) reports conflicts as C++ exceptions, and the first one
// thrown in a process has libgcc's unwinder set up its frame tables for every library then
// loaded — ~80 ms once the HIP runtime's are (tools/slow_job_probe.py: the corpus's first
// bucket whose hints meet a conflict took 80 ms, then 0.05 ms).  Both initialisers take that
// one-time cost here, with the runtime loaded, instead of the first query that conflicts.
void warm_unwinder() {
    static std::once_flag once;
    std::call_once(once, [] {
        try {
            throw std::runtime_error("unwinder warm-up");
        } catch (const std::exception&) {
        }
    });
}

// launch-geometry knobs and the device-program fold switch from the environment, read by
// both initialisers
void read_env_knobs() {
    g_device_fold = device_fold_env();
    if (const char* e = getenv("PF_WAVES_PER_CU")) {
        long v = strtol(e, nullptr, 10);
        if (v >= 8 && v <= 4096) g_knobs.waves_per_cu_full = g_knobs.waves_per_cu_early = (uint32_t)v;
    }
    if (const char* e = getenv("PF_WAVES_PER_CU_EARLY")) {  // the early-exit search alone
        long v = strtol(e, nullptr, 10);
        if (v >= 1 && v <= 4096) g_knobs.waves_per_cu_early = (uint32_t)v;
    }
    if (const char* e = getenv("PF_PROBE_MAX_SETS")) {
        long v = strtol(e, nullptr, 10);
        if (v >= 0) g_knobs.probe_max_sets = (uint32_t)v;
    }
    if (const char* e = getenv("PF_EARLY_CHUNK_GROUPS")) {
        long v = strtol(e, nullptr, 10);
        if (v >= 1 && v <= 1024) g_knobs.early_chunk_groups = (uint32_t)v;
    }
}

// one more execution context (device id, API key) with its streams and events; called under
// g_mu, inserts under g_devs_mu keeping the keys ascending
int add_dev(int id, int key, const char* who) {
    HIPCHK(hipSetDevice(id));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail("%s: device %d is %s, this build targets gfx950", who, id, prop.gcnArchName);
    std::unique_ptr<Dev> D(new Dev());
    D->id = id;
    D->key = key;
    D->num_cus = prop.multiProcessorCount;
    HIPCHK(hipStreamCreateWithFlags(&D->stream, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&D->up_stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&D->ev0));
    HIPCHK(hipEventCreate(&D->ev1));
    std::lock_guard<std::mutex> dk(g_devs_mu);
    auto at = std::upper_bound(g_devs.begin(), g_devs.end(), key,
                               [](int k, const std::unique_ptr<Dev>& e) { return k < e->key; });
    g_devs.insert(at, std::move(D));
    g_default = 0;
    return 0;
}

int pf_init(uint64_t device_mask) {
    std::lock_guard<std::mutex> lk(g_mu);
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device_mask == 0) return fail("pf_init: empty device mask");
    if (n < 64 && (device_mask >> n)) return fail("pf_init: mask %llx names devices beyond the %d visible",
                                                  (unsigned long long)device_mask, n);
    read_env_knobs();
    for (int id = 0; id < n && id < 64; ++id) {
        if (!((device_mask >> id) & 1ull) || find_dev(id)) continue;
        if (add_dev(id, id, "pf_init")) return -1;
    }
    warm_unwinder();
    return 0;
}

int pf_init_contexts(const int32_t* devices, size_t n, int32_t* ctx_out) {
    std::lock_guard<std::mutex> lk(g_mu);
    int nd = 0;
    HIPCHK(hipGetDeviceCount(&nd));
    if (!devices || !ctx_out || n == 0) return fail("pf_init_contexts: no devices");
    read_env_knobs();
    int next = PF_CONTEXT_BASE;
    for (const auto& D : g_devs) next = std::max(next, D->key + 1);
    for (size_t i = 0; i < n; ++i) {
        const int id = devices[i];
        if (id < 0 || id >= nd) return fail("pf_init_contexts: device %d of %d visible", id, nd);
        if (add_dev(id, next, "pf_init_contexts")) return -1;
        ctx_out[i] = next++;
    }
    warm_unwinder();
    return 0;
}

int pf_shutdown(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    std::lock_guard<std::mutex> dk(g_devs_mu);
    for (auto& D : g_devs) {
        hipSetDevice(D->id);
        hipDeviceSynchronize();
        {
            std::lock_guard<std::mutex> pk(g_pool_mu);
            for (auto& b : D->pool) hipFree(b.first);
            D->pool.clear();
            for (hipEvent_t e : D->ev_free) hipEventDestroy(e);
            D->ev_free.clear();
        }
        hipEventDestroy(D->ev0);
        hipEventDestroy(D->ev1);
        hipStreamDestroy(D->stream);
        if (D->up_stream) hipStreamDestroy(D->up_stream);
    }
    g_devs.clear();
    g_default = -1;
    return 0;
}

int pf_batch_create_on(int device, const uint32_t* code, size_t n_ins, const uint32_t* consts,
                       size_t n_const, const uint32_t* schema, size_t n_vars,
                       const uint32_t* parents, size_t n_parents, const pf_set_desc* descs,
                       size_t n_sets, uint64_t* handle_out) {
    // The host half — checks, the device program, the wave order, the staging copy — touches
    // no library state and runs before the lock: a caller uploading the next batch from
    // another thread (tools/full_pass.py) overlaps it with a search in progress, which holds
    // the lock until its results are back.
    Prepared pp = prepare_program(code, n_ins, consts, n_const, schema, n_vars, n_parents, descs, n_sets,
                                  g_device_fold);
    if (!pp.err.empty()) return set_err(pp.err);
    code = pp.code.data();
    n_ins = pp.code.size() / 4;
    descs = pp.descs.data();
    // the device pool: the caller's constants, then the sets' own (device_program); every
    // const_off below and on the device is an offset into it
    if (!pp.pool.empty()) {
        consts = pp.pool.data();
        n_const = pp.pool.size() / 8;
    }
    // the search kernels' wave order (narrow sets first, then longest first) and the assert sites
    WaveOrder wo = wave_order(code, descs, n_sets, pp.wide);

    // One device block, one copy: [code | consts + one zero entry | schema | parents | descs |
    // order | scratch | found], each region 256-byte aligned (found[] right after the scratch's
    // counter lines, so a search reads both back in one copy, check_collect).  The zero entry past the
    // constant pool: the generator's constant gather is issued before it knows whether the
    // set has constants (pf_eval.hip gen_var), so a set with none reads the entry at its own
    // const_off, which may be the pool's end.
    // the code region carries one zero instruction past the last END: the kernel fetches the
    // slot after an END before its dispatch leaves the program (pf_eval.hip run_program)
    const size_t o_code = 0, o_const = o_code + al(n_ins * 16 + 16), o_schema = o_const + al(n_const * 32 + 32),
                 o_par = o_schema + al(n_vars * 16), o_desc = o_par + al(n_parents * 32),
                 o_order = o_desc + al(n_sets * sizeof(pf_set_desc)), o_scr = o_order + al(n_sets * 4),
                 o_found = o_scr + PF_SCRATCH_BYTES,
                 total = o_found + al(std::max<size_t>(n_sets, 1) * 4);
    static_assert(PF_SCRATCH_BYTES % 256 == 0 && PF_COUNTER_OFF + PF_COUNTER_STRIPES * 128 == PF_SCRATCH_BYTES,
                  "found[] follows the counter lines");
    // scratch / found are cleared by every search: the copy ends at o_scr
    auto fill = [&](uint8_t* stage) {
        memset(stage, 0, o_scr);
        auto put = [&](size_t off, const void* src, size_t bytes) {
            if (bytes && src) memcpy(stage + off, src, bytes);
        };
        put(o_code, code, n_ins * 16);
        put(o_const, consts, n_const * 32);
        put(o_schema, schema, n_vars * 16);
        put(o_par, parents, n_parents * 32);
        put(o_desc, descs, n_sets * sizeof(pf_set_desc));
        put(o_order, wo.order.data(), n_sets * 4);
    };

    // No g_mu from here on either: the device lookup holds g_devs_mu (pf_init and
    // pf_init_contexts insert under it; the Dev objects themselves never move), the block comes
    // from the pool under its own lock, errors go through set_err.
    Batch* B = nullptr;
    int dev_id = -1;
    hipStream_t ups = nullptr;
    {
        Dev* Dv = nullptr;
        std::string dev_err;
        {
            std::lock_guard<std::mutex> dk(g_devs_mu);
            Dv = use_dev(device, &dev_err);
        }
        if (!Dv) return set_err(dev_err);
        if (!handle_out) return set_err("pf_batch_create: null handle_out");
        B = new Batch();
        B->device = Dv->key;
        B->n_vars = n_vars;
        B->n_sets = n_sets;
        B->max_vars = pp.max_vars;
        B->n_narrow = (size_t)std::count(pp.wide.begin(), pp.wide.end(), (uint8_t)0);
        // a set without variables counts as parented: its every candidate is candidate 0 (a
        // single query's ground keccak bucket left every such batch without the probe launch)
        B->all_parented = std::all_of(descs, descs + n_sets, [](const pf_set_desc& d) {
            return d.parent_off != PF_NO_PARENT || d.n_vars == 0;
        });
        B->h_descs.assign(descs, descs + n_sets);
        B->h_wide = std::move(pp.wide);
        B->h_sites = std::move(wo.sites);
        B->h_order = wo.order;
        if (n_const && consts) B->h_link.consts.assign(consts, consts + 8 * n_const);
        if (n_vars && schema) B->h_link.schema.assign(schema, schema + 4 * n_vars);
        if (n_parents && parents) B->h_link.parents.assign(parents, parents + 8 * n_parents);
        Block& main = B->side[kMain];
        main.mem = pool_acquire(Dv, total, &main.cap);
        if (!main.mem) {
            delete B;
            return set_err(errorf("pf_batch_create: hipMalloc(%zu) failed", total));
        }
        uint8_t* base = static_cast<uint8_t*>(main.mem);
        B->d_code = reinterpret_cast<uint4*>(base + o_code);
        B->d_consts = reinterpret_cast<uint32_t*>(base + o_const);
        B->d_schema = reinterpret_cast<uint4*>(base + o_schema);
        B->d_parents = reinterpret_cast<uint32_t*>(base + o_par);
        B->d_descs = reinterpret_cast<pf_set_desc*>(base + o_desc);
        B->d_order = reinterpret_cast<uint32_t*>(base + o_order);
        B->d_found = reinterpret_cast<uint32_t*>(base + o_found);
        B->d_scratch = reinterpret_cast<uint32_t*>(base + o_scr);
        if (event_acquire(Dv, &B->ev0) != hipSuccess || event_acquire(Dv, &B->ev1) != hipSuccess) {
            release_batch(Dv, B);
            return set_err("pf_batch_create: hipEventCreate failed");
        }
        dev_id = Dv->id;
        ups = Dv->up_stream;
    }
    // the copy itself outside g_mu, on the device's upload stream through the upload staging
    // buffer (a search holding g_mu meanwhile runs on the library stream)
    bool ok = true;
    {
        std::lock_guard<std::mutex> lk(g_up_mu);
        ok = hipSetDevice(dev_id) == hipSuccess;
        uint8_t* pin = ok ? upload_staging(o_scr) : nullptr;
        if (pin) {
            fill(pin);
            ok = hipMemcpyAsync(B->side[kMain].mem, pin, o_scr, hipMemcpyHostToDevice, ups) == hipSuccess &&
                 hipStreamSynchronize(ups) == hipSuccess;
        } else if (ok) {
            std::vector<uint8_t> stage(o_scr);
            fill(stage.data());
            ok = hipMemcpy(B->side[kMain].mem, stage.data(), o_scr, hipMemcpyHostToDevice) == hipSuccess;
        }
    }
    if (!ok) {
        // the copy may still be in flight: the block is not pooled
        free_in_flight(B->side[kMain].mem);
        B->side[kMain].mem = nullptr;
        delete B;
        return set_err(errorf("pf_batch_create: hipMemcpy of %zu bytes failed", o_scr));
    }
    *handle_out = (uint64_t)(uintptr_t)B;
    return 0;
}

int pf_batch_create(const uint32_t* code, size_t n_ins, const uint32_t* consts, size_t n_const,
                    const uint32_t* schema, size_t n_vars, const uint32_t* parents,
                    size_t n_parents, const pf_set_desc* descs, size_t n_sets,
                    uint64_t* handle_out) {
    return pf_batch_create_on(-1, code, n_ins, consts, n_const, schema, n_vars, parents, n_parents,
                              descs, n_sets, handle_out);
}

int pf_batch_free(uint64_t handle) {
    std::lock_guard<std::mutex> lk(g_mu);
    Batch* B = as_batch(handle);
    if (!B) return 0;
    Dev* D = use_dev(B->device);
    // a *_dev launch may still be reading the batch on a caller's stream: drain the stream of
    // the device's last launch (switch_stream has drained every earlier one; the library's
    // own launches are complete when their call returns, and the upload's copy when
    // pf_batch_create returned).  A whole-device synchronisation here cost every
    // single-query call a device-wide round trip.
    if (D && D->last_stream) hipStreamSynchronize(D->last_stream);
    if (D) D->last_stream = nullptr;
    release_batch(D, B);
    return 0;
}

static int found_to_host(Batch* B, const std::vector<uint32_t>& found, uint32_t* found_out,
                         uint8_t* sat_bitmap_out, pf_stats* stats) {
    uint64_t nsat = 0;
    if (sat_bitmap_out) memset(sat_bitmap_out, 0, (B->n_sets + 7) / 8);
    for (size_t s = 0; s < B->n_sets; s++) {
        if (found_out) found_out[s] = found[s];
        if (found[s] != 0xffffffffu) {
            nsat++;
            if (sat_bitmap_out) sat_bitmap_out[s / 8] |= (uint8_t)(1u << (s % 8));
        }
    }
    if (stats) stats->n_sat = nsat;
    return 0;
}

int pf_check_batch(uint64_t handle, uint64_t global_seed, uint32_t budget, uint32_t flags,
                   uint32_t timeout_ms, uint32_t* found_out, uint8_t* sat_bitmap_out,
                   pf_stats* stats) {
    std::lock_guard<std::mutex> lk(g_mu);
    Batch* B = as_batch(handle);
    if (!B) return fail("pf_check_batch: null batch");
    Dev* D = use_dev(B->device);
    if (!D || switch_stream(D, D->stream)) return -1;
    if (check_enqueue(B, global_seed, budget, flags, timeout_ms, B->d_found, D->stream)) return -1;
    std::vector<uint32_t> found;
    if (check_collect(B, D->stream, kSearchStats, stats, &found)) return -1;
    return found_to_host(B, found, found_out, sat_bitmap_out, stats);
}

int pf_check_linked(uint64_t handle, uint64_t global_seed, uint32_t budget, uint32_t flags,
                    uint32_t timeout_ms, const uint32_t* group_of, uint32_t n_groups,
                    uint32_t* found_out, pf_stats* stats) {
    std::lock_guard<std::mutex> lk(g_mu);
    Batch* B = as_batch(handle);
    if (!B) return fail("pf_check_linked: null batch");
    if (budget == 0) return fail("pf_check_linked: budget must be at least 1");
    if (!found_out) return fail("pf_check_linked: null found_out");
    if (B->n_sets == 0) return fail("pf_check_linked: the batch has no sets");
    std::vector<uint32_t> parts;
    if (failed(link_validate(B->h_descs, B->h_link, group_of, n_groups, parts))) return -1;
    const size_t ns = B->n_sets;
    const uint32_t words = groups_of(budget);
    Dev* D = use_dev(B->device);
    if (!D || switch_stream(D, D->stream)) return -1;
    hipStream_t st = D->stream;
    // the link block: [group_of: n_sets | parts: n_groups | found: n_groups | count: records | mask:
    // records], records = n_groups x ceil(budget / 64); sized to the call, grown when one needs more
    const size_t n_rec = (size_t)n_groups * words;
    const size_t o_of = 0, o_parts = o_of + al(ns * 4), o_found = o_parts + al((size_t)n_groups * 4),
                 o_count = o_found + al((size_t)n_groups * 4), o_mask = o_count + al(n_rec * 4),
                 total = o_mask + al(n_rec * 8);
    bool fresh = false;
    if (ensure(D, B, kLink, total, "pf_check_linked", &fresh)) return -1;
    if (fresh) B->l_req.clear();
    uint8_t* lb = static_cast<uint8_t*>(B->side[kLink].mem);
    LinkArgs L;
    L.group_of = reinterpret_cast<uint32_t*>(lb + o_of);
    L.parts = reinterpret_cast<uint32_t*>(lb + o_parts);
    L.found = reinterpret_cast<uint32_t*>(lb + o_found);
    L.count = reinterpret_cast<uint32_t*>(lb + o_count);
    L.mask = reinterpret_cast<unsigned long long*>(lb + o_mask);
    L.words = words;
    // the tables move with the layout (n_groups), so a call uploads them unless it repeats the
    // last call's grouping
    std::vector<uint32_t> req(group_of, group_of + ns);
    req.push_back(n_groups);
    if (req != B->l_req) {
        const size_t in_bytes = o_parts + (size_t)n_groups * 4;
        // sized for the results too: check_collect must not replace the buffer under this copy
        // (the stream orders its copies back after the upload has been consumed)
        const size_t out_bytes = kCounterBytes + (size_t)n_groups * 4;
        uint8_t* pin = pinned_staging(std::max(in_bytes, out_bytes));
        if (!pin) return fail("pf_check_linked: no pinned staging of %zu bytes", std::max(in_bytes, out_bytes));
        memcpy(pin + o_of, group_of, ns * 4);
        memcpy(pin + o_parts, parts.data(), (size_t)n_groups * 4);
        HIPCHK(hipMemcpyAsync(lb, pin, in_bytes, hipMemcpyHostToDevice, st));
        B->l_req = std::move(req);
    }
    if (check_enqueue(B, global_seed, budget, flags, timeout_ms, nullptr, st, &L, n_groups)) return -1;
    std::vector<uint32_t> found;
    pf_stats local;
    if (check_collect(B, st, kSearchStats, &local, &found, L.found, n_groups)) return -1;
    uint64_t n_sat = 0;
    for (uint32_t g = 0; g < n_groups; g++) {
        found_out[g] = found[g];
        n_sat += found[g] != 0xffffffffu;
    }
    local.n_sat = n_sat;
    if (stats) *stats = local;
    return 0;
}

int pf_check_batches(const uint64_t* handles, size_t n, uint64_t global_seed, uint32_t budget,
                     uint32_t flags, uint32_t timeout_ms, uint32_t* found_out, pf_stats* stats) {
    std::lock_guard<std::mutex> lk(g_mu);
    // 1. enqueue every batch's search on its device's stream: devices run concurrently
    for (size_t i = 0; i < n; ++i) {
        Batch* B = as_batch(handles[i]);
        if (!B) return fail("pf_check_batches: null batch %zu", i);
        Dev* D = use_dev(B->device);
        if (!D || switch_stream(D, D->stream)) return -1;
        if (check_enqueue(B, global_seed, budget, flags, timeout_ms, B->d_found, D->stream)) return -1;
    }
    // 2. gather: verdicts concatenated in handle order
    size_t off = 0;
    for (size_t i = 0; i < n; ++i) {
        Batch* B = as_batch(handles[i]);
        Dev* D = use_dev(B->device);
        if (!D) return -1;
        pf_stats* st = stats ? stats + i : nullptr;
        std::vector<uint32_t> found;
        if (check_collect(B, D->stream, kSearchStats, st, &found)) return -1;
        if (found_to_host(B, found, found_out ? found_out + off : nullptr, nullptr, st)) return -1;
        off += B->n_sets;
    }
    return 0;
}

int pf_check_batch_dev(uint64_t handle, uint64_t global_seed, uint32_t budget, uint32_t flags,
                       uint32_t timeout_ms, uint32_t* d_found, pf_stats* stats, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    Batch* B = as_batch(handle);
    if (!B) return fail("pf_check_batch_dev: null batch");
    if (!d_found) return fail("pf_check_batch_dev: null d_found");
    Dev* D = use_dev(B->device);
    if (!D) return -1;
    hipStream_t st = pick_stream(D, stream);
    if (switch_stream(D, st)) return -1;
    if (check_enqueue(B, global_seed, budget, flags, timeout_ms, d_found, st)) return -1;
    return stats ? check_collect(B, st, kSearchStats, stats) : 0;
}

int pf_materialize(uint64_t handle, uint64_t global_seed, const uint32_t* set_ids,
                   const uint32_t* cand_ids, size_t n, uint32_t* values_out) {
    std::lock_guard<std::mutex> lk(g_mu);
    Batch* B = as_batch(handle);
    if (!B) return fail("pf_materialize: null batch");
    Dev* D = use_dev(B->device);
    if (!D) return -1;
    hipStream_t st = D->stream;
    if (n == 0) return 0;
    std::vector<uint32_t> off(n);
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) {
        if (set_ids[i] >= B->n_sets) return fail("pf_materialize: set %u out of range", set_ids[i]);
        off[i] = (uint32_t)total;
        total += B->h_descs[set_ids[i]].n_vars;
    }
    if (total == 0) return 0;
    if (switch_stream(D, st)) return -1;
    // one block from the device pool ([sets | cands | offsets | values], the index arrays
    // 256-byte aligned) and the pinned staging buffer for both copies: no hipMalloc / hipFree
    // (hipFree synchronises the device) and no pageable copies per call — this runs once per
    // funnel query whose witness is not a parented candidate 0
    const size_t o_in = al(3 * n * 4), bytes = o_in + total * 32;
    Pooled blk(D, bytes);
    uint8_t* dm = blk.p;
    if (!dm) return fail("pf_materialize: hipMalloc(%zu) failed", bytes);
    uint32_t *d_sets = reinterpret_cast<uint32_t*>(dm), *d_cands = d_sets + n, *d_off = d_cands + n,
             *d_out = reinterpret_cast<uint32_t*>(dm + o_in);
    uint8_t* pin = pinned_staging(std::max<size_t>(3 * n * 4, total * 32));
    HIPTRY("pf_materialize",
           copy_in(dm, pin, {{0, set_ids, n * 4}, {n * 4, cand_ids, n * 4}, {2 * n * 4, off.data(), n * 4}}, st));
    const uint32_t mv = std::max<uint32_t>(B->max_vars, 1u);
    const uint64_t threads = (uint64_t)n * mv;
    hipLaunchKernelGGL(pf_materialize_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st, B->d_descs,
                       B->d_code, B->d_consts, B->d_schema, B->d_parents, global_seed, d_sets, d_cands, d_off,
                       (uint32_t)n, mv, d_out);
    HIPTRY("pf_materialize", hipGetLastError());
    HIPTRY("pf_materialize", copy_out(values_out, dm + o_in, total * 32, pin, st));
    blk.release();
    return 0;
}

int pf_climb_batch(uint64_t handle, uint64_t global_seed, uint32_t rounds, uint32_t per_round,
                   uint32_t timeout_ms, const uint32_t* set_ids, size_t n, uint32_t* status_out,
                   uint32_t* score_out, uint32_t* round_out, uint32_t* values_out, pf_stats* stats) {
    return pf_climb_batch_scored(handle, global_seed, rounds, per_round, PF_CLIMB_SCORE_SITES, timeout_ms, set_ids,
                                 n, status_out, score_out, round_out, values_out, stats);
}

int pf_climb_batch_scored(uint64_t handle, uint64_t global_seed, uint32_t rounds, uint32_t per_round,
                          uint32_t score, uint32_t timeout_ms, const uint32_t* set_ids, size_t n,
                          uint32_t* status_out, uint32_t* score_out, uint32_t* round_out,
                          uint32_t* values_out, pf_stats* stats) {
    std::lock_guard<std::mutex> lk(g_mu);
    Batch* B = as_batch(handle);
    if (!B) return fail("pf_climb_batch: null batch");
    if (score != PF_CLIMB_SCORE_SITES && score != PF_CLIMB_SCORE_TREE)
        return fail("pf_climb_batch: unknown score %u", score);
    if (rounds == 0) return fail("pf_climb_batch: rounds must be at least 1");
    if (per_round == 0) return fail("pf_climb_batch: per_round must be at least 1");
    const size_t ns = B->n_sets;
    if (failed(check_request("pf_climb_batch", ns, set_ids, n))) return -1;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return 0;
    const uint32_t groups = groups_of(per_round);
    if (failed(check_items("pf_climb_batch", n, groups))) return -1;
    Dev* D = use_dev(B->device);
    if (!D) return -1;
    hipStream_t st = D->stream;
    if (switch_stream(D, st)) return -1;

    // the climb block: [working descs | working schema | parent buffers A, B | states | per set:
    // first parent row, witness score | this call's set ids, 8-register sets first]
    std::vector<uint32_t> wvoff(ns);
    size_t n_wvars = 0;
    for (size_t s = 0; s < ns; s++) {
        wvoff[s] = (uint32_t)n_wvars;
        n_wvars += B->h_descs[s].n_vars;
    }
    if (n_wvars > 0xffffffffull / 8) return fail("pf_climb_batch: %zu variables", n_wvars);
    const size_t o_wd = 0, o_ws = o_wd + al(ns * sizeof(pf_set_desc)), o_p0 = o_ws + al(n_wvars * 16 + 16),
                 o_p1 = o_p0 + al(n_wvars * 32 + 32), o_st = o_p1 + al(n_wvars * 32 + 32),
                 o_tab = o_st + al(ns * sizeof(pf_climb_set)), total = o_tab + al(3 * ns * 4);
    if (ensure(D, B, kClimb, total, "pf_climb_batch")) return -1;
    uint8_t* cb = static_cast<uint8_t*>(B->side[kClimb].mem);
    pf_set_desc* d_wdescs = reinterpret_cast<pf_set_desc*>(cb + o_wd);
    uint4* d_wschema = reinterpret_cast<uint4*>(cb + o_ws);
    uint32_t* d_par[2] = {reinterpret_cast<uint32_t*>(cb + o_p0), reinterpret_cast<uint32_t*>(cb + o_p1)};
    pf_climb_set* d_state = reinterpret_cast<pf_climb_set*>(cb + o_st);
    uint32_t* d_wvoff = reinterpret_cast<uint32_t*>(cb + o_tab);
    uint32_t *d_target = d_wvoff + ns, *d_req = d_target + ns;

    // this call's sets in launch order: the 8-register ones, then the 16-register ones
    std::vector<uint32_t> req;
    const size_t n_narrow = request_order(B->h_wide, set_ids, n, req);
    std::vector<uint32_t> target(ns);
    for (size_t s = 0; s < ns; s++) target[s] = PF_CLIMB_HOLDS * B->h_sites[s];

    constexpr size_t cbytes = kCounterBytes;
    const size_t in_bytes = 3 * ns * 4, out_bytes = cbytes + ns * sizeof(pf_climb_set) + n_wvars * 32;
    uint8_t* pin = pinned_staging(std::max(in_bytes, out_bytes));
    if (!pin) return fail("pf_climb_batch: no pinned staging of %zu bytes", std::max(in_bytes, out_bytes));
    memcpy(pin, wvoff.data(), ns * 4);
    memcpy(pin + ns * 4, target.data(), ns * 4);
    memset(pin + 2 * ns * 4, 0, ns * 4);
    memcpy(pin + 2 * ns * 4, req.data(), n * 4);
    HIPCHK(hipMemcpyAsync(d_wvoff, pin, in_bytes, hipMemcpyHostToDevice, st));

    constexpr uint32_t n_queue = 2 * PF_EARLY_QUEUES * PF_EARLY_QUEUE_STRIDE;  // the heads of both parts
    if (reset_scratch(B, st, B->d_found, 0u)) return -1;  // found[] is left alone
    hipLaunchKernelGGL(pf_climb_init_kernel, dim3((uint32_t)n), dim3(64), 0, st, B->d_descs, B->d_schema, d_req,
                       d_wvoff, d_target, d_wdescs, d_wschema, d_state);
    HIPCHK(hipGetLastError());
    const uint64_t deadline = timeout_ms ? (uint64_t)timeout_ms * 100000ull : 0ull;  // 100 MHz
    // the rounds, back to back on the stream: nothing here waits for the device
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint64_t gs = global_seed + (uint64_t)(r + 1u) * PF_CLIMB_SEED_MUL;
        const pf_set_desc* descs_r = r ? d_wdescs : B->d_descs;
        const uint4* schema_r = r ? d_wschema : B->d_schema;
        const uint32_t* parents_r = r ? d_par[r & 1u] : B->d_parents;
        for (int part = 0; part < 2; ++part) {
            const size_t first = part ? n_narrow : 0, np = part ? n - n_narrow : n_narrow;
            if (np == 0) continue;
            const Grid g = group_grid(g_knobs, D->num_cus, np, groups);
            const auto kernel = score == PF_CLIMB_SCORE_TREE ? (part == 0 ? pf_climb_tree_kernel : pf_climb_tree_r16_kernel)
                                                             : (part == 0 ? pf_climb_kernel : pf_climb_r16_kernel);
            hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(64 * PF_SEARCH_WG_WAVES), 0, st, descs_r, d_req + first,
                               (uint32_t)np, B->d_code, B->d_consts, schema_r, parents_r, gs, per_round, groups,
                               r ? 1u : 0u, deadline, B->t0(), d_state, B->counters(), B->queue(0, part));
            HIPCHK(hipGetLastError());
        }
        // the adopt kernel clears the heads for the next round: the first part's, n_queue words on
        hipLaunchKernelGGL(pf_climb_adopt_kernel, dim3((uint32_t)n), dim3(64), 0, st, descs_r, d_wdescs, d_req,
                           B->d_code, B->d_consts, schema_r, parents_r, gs, r, d_par[r & 1u], d_par[(r + 1u) & 1u],
                           d_state, B->queue(0, 0), n_queue);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(B->ev1, st));
    // counters, states and the final assignments (A_R, in buffer R & 1) in the staging buffer;
    // the stream orders these copies after the upload above has been consumed
    HIPCHK(hipMemcpyAsync(pin, B->counter_lines(), cbytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(pin + cbytes, d_state, ns * sizeof(pf_climb_set), hipMemcpyDeviceToHost, st));
    if (n_wvars)
        HIPCHK(hipMemcpyAsync(pin + cbytes + ns * sizeof(pf_climb_set), d_par[rounds & 1u], n_wvars * 32,
                              hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const pf_climb_set* hst = reinterpret_cast<const pf_climb_set*>(pin + cbytes);
    const uint32_t* hv = reinterpret_cast<const uint32_t*>(pin + cbytes + ns * sizeof(pf_climb_set));
    uint64_t n_sat = 0;
    size_t off = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t s = set_ids[i];
        if (status_out) status_out[i] = hst[s].status;
        if (score_out) score_out[i] = hst[s].score;
        if (round_out) round_out[i] = hst[s].round;
        n_sat += hst[s].status == PF_CLIMB_WITNESS;
        const size_t nv = B->h_descs[s].n_vars;
        if (values_out && nv) memcpy(values_out + off * 8, hv + (size_t)wvoff[s] * 8, nv * 32);
        off += nv;
    }
    return stats ? fill_stats(B, reinterpret_cast<const unsigned long long*>(pin), kSideStats, n_sat, stats) : 0;
}

int pf_batch_site_counts(uint64_t handle, const uint32_t* set_ids, size_t n, uint32_t* counts_out) {
    std::lock_guard<std::mutex> lk(g_mu);
    Batch* B = as_batch(handle);
    if (!B) return fail("pf_batch_site_counts: null batch");
    if (n && (!set_ids || !counts_out)) return fail("pf_batch_site_counts: null argument");
    for (size_t i = 0; i < n; i++) {
        if (set_ids[i] >= B->n_sets)
            return fail("pf_batch_site_counts: set %u out of range (%zu sets)", set_ids[i], B->n_sets);
        counts_out[i] = B->h_sites[set_ids[i]];
    }
    return 0;
}

int pf_census_batch(uint64_t handle, uint64_t global_seed, uint32_t budget, uint32_t timeout_ms,
                    const uint32_t* set_ids, size_t n, uint32_t* holds_out, uint32_t* alive_out,
                    uint32_t* sole_out, uint32_t* best_fails_out, uint32_t* best_cand_out,
                    uint32_t* status_out, pf_stats* stats) {
    std::lock_guard<std::mutex> lk(g_mu);
    Batch* B = as_batch(handle);
    if (!B) return fail("pf_census_batch: null batch");
    if (budget == 0) return fail("pf_census_batch: budget must be at least 1");
    const size_t ns = B->n_sets;
    const auto few_sites = [&](uint32_t s) {
        return B->h_sites[s] > PF_CENSUS_MAX_SITES
                   ? errorf("pf_census_batch: set %u has %u sites (at most %u)", s, B->h_sites[s], PF_CENSUS_MAX_SITES)
                   : std::string();
    };
    if (failed(check_request("pf_census_batch", ns, set_ids, n, few_sites))) return -1;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return 0;
    const uint32_t groups = groups_of(budget);
    if (failed(check_items("pf_census_batch", n, groups))) return -1;
    Dev* D = use_dev(B->device);
    if (!D) return -1;
    hipStream_t st = D->stream;
    if (switch_stream(D, st)) return -1;

    // the census block: [states | rows: per set holds, alive, sole | per set: first row, sites |
    // this call's set ids, 8-register sets first].  Its size depends on the batch alone.
    std::vector<uint32_t> row_off(ns);
    uint64_t n_rows = 0;
    for (size_t s = 0; s < ns; s++) {
        row_off[s] = (uint32_t)n_rows;
        n_rows += 3ull * B->h_sites[s];
    }
    if (n_rows + ns > 0xffffffffull) return fail("pf_census_batch: %llu row entries", (unsigned long long)n_rows);
    const size_t o_st = 0, o_rows = o_st + al(ns * sizeof(pf_census_set)), o_tab = o_rows + al((size_t)n_rows * 4 + 4),
                 total = o_tab + al(3 * ns * 4);
    if (ensure(D, B, kCensus, total, "pf_census_batch")) return -1;
    uint8_t* sb = static_cast<uint8_t*>(B->side[kCensus].mem);
    pf_census_set* d_state = reinterpret_cast<pf_census_set*>(sb + o_st);
    uint32_t* d_rows = reinterpret_cast<uint32_t*>(sb + o_rows);
    uint32_t* d_rowoff = reinterpret_cast<uint32_t*>(sb + o_tab);
    uint32_t *d_nsites = d_rowoff + ns, *d_req = d_nsites + ns;

    // this call's sets in launch order: the 8-register ones, then the 16-register ones
    std::vector<uint32_t> req;
    const size_t n_narrow = request_order(B->h_wide, set_ids, n, req);

    constexpr size_t cbytes = kCounterBytes;
    const size_t in_bytes = 3 * ns * 4, out_bytes = cbytes + ns * sizeof(pf_census_set) + (size_t)n_rows * 4;
    uint8_t* pin = pinned_staging(std::max(in_bytes, out_bytes));
    if (!pin) return fail("pf_census_batch: no pinned staging of %zu bytes", std::max(in_bytes, out_bytes));
    memcpy(pin, row_off.data(), ns * 4);
    memcpy(pin + ns * 4, B->h_sites.data(), ns * 4);
    memset(pin + 2 * ns * 4, 0, ns * 4);
    memcpy(pin + 2 * ns * 4, req.data(), n * 4);
    HIPCHK(hipMemcpyAsync(d_rowoff, pin, in_bytes, hipMemcpyHostToDevice, st));

    // the launches, back to back on the stream: the scratch reset (found[] is left alone), the
    // census block's reset, the two parts' census launches; nothing here waits for the device
    if (reset_scratch(B, st, B->d_found, 0u)) return -1;  // found[] is left alone
    {
        const uint64_t cells = n_rows + ns;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((cells + 255u) / 256u, 1024u);
        hipLaunchKernelGGL(pf_census_init_kernel, dim3(blocks), dim3(256), 0, st, d_rowoff, d_nsites, (uint32_t)ns,
                           d_state, d_rows, (uint32_t)n_rows);
        HIPCHK(hipGetLastError());
    }
    const uint64_t deadline = timeout_ms ? (uint64_t)timeout_ms * 100000ull : 0ull;  // 100 MHz
    for (int part = 0; part < 2; ++part) {
        const size_t first = part ? n_narrow : 0, np = part ? n - n_narrow : n_narrow;
        if (np == 0) continue;
        const Grid g = group_grid(g_knobs, D->num_cus, np, groups);
        hipLaunchKernelGGL(part == 0 ? pf_census_kernel : pf_census_r16_kernel, dim3(g.blocks),
                           dim3(64 * PF_SEARCH_WG_WAVES), 0, st, B->d_descs, d_req + first, (uint32_t)np, B->d_code,
                           B->d_consts, B->d_schema, B->d_parents, global_seed, budget, groups, deadline, B->t0(),
                           d_state, d_rows, B->counters(), B->queue(0, part));
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(B->ev1, st));
    // counters, states and rows in the staging buffer; the stream orders these copies after the
    // upload above has been consumed
    HIPCHK(hipMemcpyAsync(pin, B->counter_lines(), cbytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(pin + cbytes, d_state, ns * sizeof(pf_census_set), hipMemcpyDeviceToHost, st));
    if (n_rows)
        HIPCHK(hipMemcpyAsync(pin + cbytes + ns * sizeof(pf_census_set), d_rows, (size_t)n_rows * 4,
                              hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const pf_census_set* hst = reinterpret_cast<const pf_census_set*>(pin + cbytes);
    const uint32_t* hr = reinterpret_cast<const uint32_t*>(pin + cbytes + ns * sizeof(pf_census_set));
    uint64_t n_sat = 0;
    size_t off = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t s = set_ids[i];
        const size_t k = B->h_sites[s];
        const bool is_cut = hst[s].cut != 0u;
        const uint32_t* r = hr + row_off[s];
        uint32_t* outs[3] = {holds_out, alive_out, sole_out};
        for (int a = 0; a < 3; a++) {
            if (!outs[a] || !k) continue;
            if (is_cut) memset(outs[a] + off, 0, k * 4);
            else memcpy(outs[a] + off, r + (size_t)a * k, k * 4);
        }
        off += k;
        const uint32_t bf = is_cut ? 0xffffffffu : (uint32_t)(hst[s].best >> 32);
        const uint32_t bc = is_cut ? 0xffffffffu : (uint32_t)hst[s].best;
        if (best_fails_out) best_fails_out[i] = bf;
        if (best_cand_out) best_cand_out[i] = bc;
        if (status_out) status_out[i] = is_cut ? PF_CENSUS_CUT : PF_CENSUS_DONE;
        n_sat += bf == 0u;
    }
    return stats ? fill_stats(B, reinterpret_cast<const unsigned long long*>(pin), kSideStats, n_sat, stats) : 0;
}

static int eval_launch(Batch* B, uint32_t set, const uint32_t* d_soa, uint32_t n_cand,
                       uint8_t* d_out, hipStream_t st) {
    if (set >= B->n_sets) return fail("eval: set %u out of range", set);
    if (n_cand == 0) return 0;
    hipLaunchKernelGGL(pf_eval_soa_kernel, dim3((n_cand + 255) / 256), dim3(256), 0, st, B->d_descs,
                       set, B->d_code, B->d_consts, B->d_schema, B->d_parents, d_soa, n_cand, d_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int pf_eval_assignments(uint64_t handle, uint32_t set, const uint32_t* soa, uint32_t n_cand,
                        uint8_t* sat_out) {
    std::lock_guard<std::mutex> lk(g_mu);
    Batch* B = as_batch(handle);
    if (!B) return fail("pf_eval_assignments: null batch");
    Dev* D = use_dev(B->device);
    if (!D) return -1;
    hipStream_t st = D->stream;
    if (set >= B->n_sets) return fail("eval: set %u out of range", set);
    if (n_cand == 0) return 0;
    const size_t nv = std::max<uint32_t>(B->h_descs[set].n_vars, 1u);
    const size_t bytes = nv * 8 * (size_t)n_cand * 4;
    if (switch_stream(D, st)) return -1;
    // one pooled block [assignments | verdicts] and the pinned staging buffer for both
    // copies (the GPU-resident ModelCache calls this once per quick-sat query: no hipMalloc /
    // hipFree, no pageable copies — pf_materialize's pattern)
    const size_t o_out = al(bytes), total = o_out + n_cand;
    Pooled blk(D, total);
    uint8_t* dm = blk.p;
    if (!dm) return fail("pf_eval_assignments: hipMalloc(%zu) failed", total);
    uint8_t* pin = pinned_staging(std::max<size_t>(bytes, n_cand));
    HIPTRY("pf_eval_assignments", copy_in(dm, pin, {{0, soa, bytes}}, st));
    if (eval_launch(B, set, reinterpret_cast<const uint32_t*>(dm), n_cand, dm + o_out, st)) return -1;
    HIPTRY("pf_eval_assignments", copy_out(sat_out, dm + o_out, n_cand, pin, st));
    blk.release();
    return 0;
}

// pf_eval_program / pf_eval_programs: the program(s) validated and rewritten exactly as by
// pf_batch_create (prepare_program), one pooled block [code | consts + zero entry | schema |
// descs | assignments | verdicts] and one copy each way through the pinned staging buffer;
// the stream is synchronised, not the device (no batch object, no events): the quick-sat call
// of the GPU-resident ModelCache, once or twice per objective-free query
// (mythril_amd/model_cache.py)
static int eval_programs(const char* who, int device, const uint32_t* code, size_t n_ins, const uint32_t* consts,
                         size_t n_const, const uint32_t* schema, size_t n_vars, const pf_set_desc* descs,
                         size_t n_sets, const uint32_t* soa, uint32_t n_cand, uint8_t* sat_out) {
    Dev* D = use_dev(device);
    if (!D) return -1;
    if (n_cand == 0 || n_sets == 0) return 0;
    if (!code || !sat_out || !descs || (n_vars && !soa)) return fail("%s: null argument", who);
    if (n_sets > 65535) return fail("%s: %zu programs (at most 65535)", who, n_sets);
    // (under g_mu, as every caller of this is)
    const Prepared pp = prepare_program(code, n_ins, consts, n_const, schema, n_vars, 0, descs, n_sets, g_device_fold);
    if (!pp.err.empty()) return fail("%s", pp.err.c_str());
    const std::vector<uint32_t>& code_out = pp.code;
    const std::vector<pf_set_desc>& descs_out = pp.descs;
    if (!pp.pool.empty()) {  // the device pool (device_program): descs_out index into it
        consts = pp.pool.data();
        n_const = pp.pool.size() / 8;
    }
    const size_t nv = std::max<size_t>(n_vars, 1), n_dev = code_out.size() / 4, n_out = n_sets * (size_t)n_cand;
    const size_t soa_bytes = nv * 8 * (size_t)n_cand * 4;
    const size_t o_code = 0, o_const = al(n_dev * 16 + 16), o_schema = o_const + al(n_const * 32 + 32),  // + the pad slot
                 o_desc = o_schema + al(nv * 16), o_soa = o_desc + al(n_sets * sizeof(pf_set_desc)),
                 o_out = o_soa + al(soa_bytes), total = o_out + n_out;
    uint8_t* pin = pinned_staging(std::max<size_t>(o_out, n_out));
    if (!pin) return fail("%s: no pinned staging buffer", who);
    memset(pin, 0, o_out);
    memcpy(pin + o_code, code_out.data(), n_dev * 16);
    if (n_const) memcpy(pin + o_const, consts, n_const * 32);
    if (n_vars) memcpy(pin + o_schema, schema, n_vars * 16);
    memcpy(pin + o_desc, descs_out.data(), n_sets * sizeof(pf_set_desc));
    if (n_vars) memcpy(pin + o_soa, soa, soa_bytes);
    hipStream_t st = D->stream;
    if (switch_stream(D, st)) return -1;
    Pooled blk(D, total);
    uint8_t* dm = blk.p;
    if (!dm) return fail("%s: hipMalloc(%zu) failed", who, total);
    HIPTRY(who, hipMemcpyAsync(dm, pin, o_out, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pf_eval_soa_sets_kernel, dim3((n_cand + 63) / 64, (unsigned)n_sets), dim3(64), 0, st,
                       reinterpret_cast<const pf_set_desc*>(dm + o_desc), reinterpret_cast<const uint4*>(dm + o_code),
                       reinterpret_cast<const uint32_t*>(dm + o_const), reinterpret_cast<const uint4*>(dm + o_schema),
                       reinterpret_cast<const uint32_t*>(dm + o_soa), n_cand, dm + o_out);
    HIPTRY(who, hipGetLastError());
    HIPTRY(who, copy_out(sat_out, dm + o_out, n_out, pin, st));
    blk.release();
    return 0;
}

int pf_eval_program(int device, const uint32_t* code, size_t n_ins, const uint32_t* consts, size_t n_const,
                    const uint32_t* schema, size_t n_vars, const uint32_t* soa, uint32_t n_cand,
                    uint8_t* sat_out) {
    std::lock_guard<std::mutex> lk(g_mu);
    const pf_set_desc d0{0u, (uint32_t)n_ins, 0u, (uint32_t)n_const, 0u, (uint32_t)n_vars, 0u, PF_NO_PARENT};
    return eval_programs("pf_eval_program", device, code, n_ins, consts, n_const, schema, n_vars, &d0, 1, soa,
                         n_cand, sat_out);
}

int pf_eval_programs(int device, const uint32_t* code, size_t n_ins, const uint32_t* consts, size_t n_const,
                     const uint32_t* schema, size_t n_vars, const pf_set_desc* descs, size_t n_sets,
                     const uint32_t* soa, uint32_t n_cand, uint8_t* sat_out) {
    std::lock_guard<std::mutex> lk(g_mu);
    return eval_programs("pf_eval_programs", device, code, n_ins, consts, n_const, schema, n_vars, descs, n_sets,
                         soa, n_cand, sat_out);
}

int pf_eval_assignments_dev(uint64_t handle, uint32_t set, const uint32_t* d_soa,
                            uint32_t n_cand, uint8_t* d_sat_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    Batch* B = as_batch(handle);
    if (!B) return fail("pf_eval_assignments_dev: null batch");
    Dev* D = use_dev(B->device);
    if (!D) return -1;
    if (switch_stream(D, pick_stream(D, stream))) return -1;
    return eval_launch(B, set, d_soa, n_cand, d_sat_out, pick_stream(D, stream));
}

// ---- stream: explicit assignments through every requested set (stream contract) ------------
// What both stream entry points check before anything is launched.  -1: an error (g_err set);
// 0: nothing to do; 1: go on.
static int stream_check(const char* who, Batch* B, const uint32_t* set_ids, size_t n, const void* soa,
                        uint32_t n_cand, uint32_t flags, const void* bits, const void* first, const void* count,
                        pf_stats* stats) {
    if (!B) return fail("%s: null batch", who);
    if (flags & ~PF_FLAG_SHORTCIRCUIT) return fail("%s: unknown flags 0x%x (PF_FLAG_SHORTCIRCUIT only)", who, flags);
    if (failed(check_request(who, B->n_sets, set_ids, n))) return -1;
    const bool vars = std::any_of(set_ids, set_ids + n, [&](uint32_t s) { return B->h_descs[s].n_vars != 0; });
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0 || n_cand == 0) return 0;  // no output has an entry to write
    if (!bits && !first && !count) return fail("%s: every output is null", who);
    if (vars && !soa) return fail("%s: null assignments", who);
    return failed(check_items(who, n, groups_of(n_cand))) ? -1 : 1;
}

// Enqueue one stream call on st (B's device current, the request checked): the request's tables
// (uploaded only when they differ from the last call's), the reset, the narrow and the wide
// launch, between B's events.
static int stream_enqueue(Dev* D, Batch* B, const uint32_t* set_ids, size_t n, const uint32_t* d_soa,
                          uint32_t n_cand, uint32_t flags, uint64_t* d_bits, uint32_t* d_first, uint32_t* d_count,
                          hipStream_t st) {
    bool fresh = false;
    if (ensure(D, B, kStream, std::max<size_t>(2 * B->n_sets * 4, 256), "pf_eval_batch", &fresh)) return -1;
    if (fresh) B->e_req.clear();
    // this call's sets in launch order — d_order's: the 8-register ones, then the 16-register
    // ones, each part longest first — and each one's place in the request
    std::vector<uint32_t> tab;
    const size_t n_narrow = batch_order(B->h_order, B->h_wide, set_ids, n, tab);
    uint32_t* d_req = static_cast<uint32_t*>(B->side[kStream].mem);
    uint32_t* d_pos = d_req + n;
    if (tab != B->e_req) {
        // a copy from pageable memory: drained before the table goes out of scope.  Only a call
        // whose request differs from the batch's last one pays it.
        B->e_req.clear();
        HIPCHK(hipMemcpyAsync(d_req, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        B->e_req = std::move(tab);
    }
    const uint32_t groups = groups_of(n_cand);
    // the caller's first[], or the batch's found[] (n <= n_sets entries): the kernels count the
    // sets with a witness through it
    uint32_t* first = d_first ? d_first : B->d_found;
    {
        const uint32_t nz = PF_SCRATCH_BYTES / 4;
        const uint32_t blocks = std::min<uint32_t>((nz + (uint32_t)n + 255u) / 256u, 1024u);
        hipLaunchKernelGGL(pf_stream_reset_kernel, dim3(blocks), dim3(256), 0, st, B->d_scratch, nz, first, d_count,
                           (uint32_t)n);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(B->ev0, st));
    // PF_STREAM_CHUNK_GROUPS (read on every call, for tests and sweeps): the groups per item
    uint64_t chunk_env = 0;
    if (const char* e = getenv("PF_STREAM_CHUNK_GROUPS")) {
        const long v = strtol(e, nullptr, 10);
        if (v >= 1 && v <= 65536) chunk_env = (uint64_t)v;
    }
    for (int part = 0; part < 2; ++part) {
        const size_t begin = part ? n_narrow : 0, np = part ? n - n_narrow : n_narrow;
        if (np == 0) continue;
        const Grid g = stream_grid(g_knobs, D->num_cus, np, groups, chunk_env);
        hipLaunchKernelGGL(part == 0 ? pf_eval_stream_kernel : pf_eval_stream_r16_kernel, dim3(g.blocks),
                           dim3(64 * PF_SEARCH_WG_WAVES), 0, st, B->d_descs, d_req + begin, d_pos + begin, (uint32_t)np,
                           B->d_code, B->d_consts, B->d_schema, d_soa, n_cand, groups, g.per, flags,
                           reinterpret_cast<unsigned long long*>(d_bits), first, d_count, B->counters(),
                           B->queue(0, part));
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(B->ev1, st));
    return 0;
}

int pf_eval_batch_dev(uint64_t handle, const uint32_t* set_ids, size_t n, const uint32_t* d_soa, uint32_t n_cand,
                      uint32_t flags, uint64_t* d_bits, uint32_t* d_first, uint32_t* d_count, pf_stats* stats,
                      void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    Batch* B = as_batch(handle);
    const int go = stream_check("pf_eval_batch_dev", B, set_ids, n, d_soa, n_cand, flags, d_bits, d_first, d_count,
                                stats);
    if (go <= 0) return go;
    Dev* D = use_dev(B->device);
    if (!D) return -1;
    hipStream_t st = pick_stream(D, stream);
    if (switch_stream(D, st)) return -1;
    if (stream_enqueue(D, B, set_ids, n, d_soa, n_cand, flags, d_bits, d_first, d_count, st)) return -1;
    return stats ? check_collect(B, st, kStreamStats, stats) : 0;
}

int pf_eval_batch(uint64_t handle, const uint32_t* set_ids, size_t n, const uint32_t* soa, uint32_t n_cand,
                  uint32_t flags, uint64_t* bits_out, uint32_t* first_out, uint32_t* count_out, pf_stats* stats) {
    std::lock_guard<std::mutex> lk(g_mu);
    Batch* B = as_batch(handle);
    const int go = stream_check("pf_eval_batch", B, set_ids, n, soa, n_cand, flags, bits_out, first_out, count_out,
                                stats);
    if (go <= 0) return go;
    Dev* D = use_dev(B->device);
    if (!D) return -1;
    hipStream_t st = D->stream;
    if (switch_stream(D, st)) return -1;
    // one pooled block [assignments | bits | first | count] and the pinned staging buffer for both
    // copies (pf_eval_assignments' pattern)
    const size_t words = ((size_t)n_cand + 63) / 64;
    const size_t soa_bytes = soa ? B->n_vars * 8 * (size_t)n_cand * 4 : 0;
    const size_t o_bits = al(std::max<size_t>(soa_bytes, 4)), o_first = o_bits + al(n * words * 8),
                 o_count = o_first + al(n * 4), total = o_count + al(n * 4), out_bytes = total - o_bits;
    Pooled blk(D, total);
    uint8_t* dm = blk.p;
    if (!dm) return fail("pf_eval_batch: hipMalloc(%zu) failed", total);
    uint8_t* pin = pinned_staging(std::max(soa_bytes, out_bytes));
    if (!pin) return fail("pf_eval_batch: HIP call failed");
    if (soa_bytes) HIPTRY("pf_eval_batch", copy_in(dm, pin, {{0, soa, soa_bytes}}, st));
    if (stream_enqueue(D, B, set_ids, n, reinterpret_cast<const uint32_t*>(dm), n_cand, flags,
                       bits_out ? reinterpret_cast<uint64_t*>(dm + o_bits) : nullptr,
                       first_out ? reinterpret_cast<uint32_t*>(dm + o_first) : nullptr,
                       count_out ? reinterpret_cast<uint32_t*>(dm + o_count) : nullptr, st))
        return -1;
    // the staging buffer is reused for the results, [bits | first | count] as in the block: the
    // stream orders the copy after the kernels, which ran after the copy-in
    HIPTRY("pf_eval_batch", hipMemcpyAsync(pin, dm + o_bits, out_bytes, hipMemcpyDeviceToHost, st));
    HIPTRY("pf_eval_batch", hipStreamSynchronize(st));
    if (bits_out) memcpy(bits_out, pin, n * words * 8);
    if (first_out) memcpy(first_out, pin + (o_first - o_bits), n * 4);
    if (count_out) memcpy(count_out, pin + (o_count - o_bits), n * 4);
    blk.release();
    return stats ? check_collect(B, st, kStreamStats, stats) : 0;
}

int pf_keccak256_batch(const uint8_t* data, const uint64_t* offsets, size_t n, uint8_t* out32) {
    std::lock_guard<std::mutex> lk(g_mu);
    Dev* D = use_dev(-1);
    if (!D) return -1;
    hipStream_t st = D->stream;
    if (n == 0) return 0;
    for (size_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return fail("keccak: offsets not monotone at %zu", i);
    const uint64_t total = offsets[n];
    if (switch_stream(D, st)) return -1;
    // one pooled block [offsets | messages | digests] and one copy each way through the
    // pinned staging buffer (a concretisation call hashes a handful of preimages: three
    // hipMalloc / hipFree pairs and pageable copies were most of its latency)
    const size_t o_off = 0, o_data = al((n + 1) * 8), o_out = o_data + al(total ? total : 8),
                 all = o_out + n * 32;
    Pooled blk(D, all);
    uint8_t* dm = blk.p;
    if (!dm) return fail("pf_keccak256_batch: hipMalloc(%zu) failed", all);
    uint8_t* pin = pinned_staging(std::max<size_t>(o_out, n * 32));
    HIPTRY("pf_keccak256_batch", copy_in(dm, pin, {{o_off, offsets, (n + 1) * 8}, {o_data, data, total}}, st));
    hipLaunchKernelGGL(pf_keccak_var_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, dm + o_data,
                       reinterpret_cast<const uint64_t*>(dm + o_off), (uint64_t)n, dm + o_out);
    HIPTRY("pf_keccak256_batch", hipGetLastError());
    HIPTRY("pf_keccak256_batch", copy_out(out32, dm + o_out, n * 32, pin, st));
    blk.release();
    return 0;
}

int pf_keccak256_fixed_dev(const uint8_t* d_data, uint32_t len, size_t n, uint8_t* d_out32,
                           float* kernel_ms, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    Dev* D = use_dev(-1);
    if (!D) return -1;
    if (n == 0) return 0;
    hipStream_t st = pick_stream(D, stream);
    if (switch_stream(D, st)) return -1;
    HIPCHK(hipEventRecord(D->ev0, st));
    const bool fast = (len % 16u) == 0u && len < 136u && (((uintptr_t)d_data) & 15u) == 0u;
    hipLaunchKernelGGL(fast ? pf_keccak_fixed_kernel : pf_keccak_stride_kernel,
                       dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, d_data, len, (uint64_t)n, d_out32);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(D->ev1, st));
    if (kernel_ms) {
        HIPCHK(hipEventSynchronize(D->ev1));
        HIPCHK(hipEventElapsedTime(kernel_ms, D->ev0, D->ev1));
    }
    return 0;
}

}  // extern "C"
