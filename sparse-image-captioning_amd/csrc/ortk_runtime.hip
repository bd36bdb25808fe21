// ortk_runtime.hip — the library's process-wide state, all of it: the tuning switches (ortk_tuning), the per-(device, function)
// dynamic-LDS attribute cache, and the opt-in per-launch profiling registry that ortk_gemm, the chains, the decoder stack and the
// grouped weight gradients record into.  Nothing here launches a kernel.
#include <mutex>
#include <vector>
#include "ortk_internal.h"

// ------------------------------------------------------------------------------------------------ tuning switches
namespace ortk {
// The product path, field by field (ortk.h documents each; a field added to the header starts at 0 here until it is given a line).
static ortk_tuning tuning_defaults() {
    ortk_tuning t{};
    t.gemm_t64 = 640;
    t.attn_impl = 0;
    t.attn16_min_lq = 33;
    t.side_stream = 1;
    t.row_chain = 1;
    t.chain_wide = 1;
    t.spmm_alias = 1;
    t.f32_split = 1;
    t.wgrad_wgs = 384;
    t.wgrad_group = 3;
    t.wgrad_group_splitk = 0;
    t.wgrad_group_wgs = 96;
    t.wgrad_group_tail = 1;
    t.feats_bf16 = 1;
    t.ln_fuse = 0;
    t.samp_epilogue = 1;
    t.gemm_epilogue = 0;
    t.attn16_short = 1;
    t.attn16_block = 1;
    return t;
}
static ortk_tuning g_tuning = tuning_defaults();
const ortk_tuning& tuning() { return g_tuning; }
}  // namespace ortk

extern "C" void ortk_get_tuning(ortk_tuning* out) { if (out) *out = ortk::g_tuning; }
extern "C" int ortk_set_tuning(const ortk_tuning* t) {
    if (!t) return ORTK_EINVAL;
    auto in = [](int32_t v, int32_t lo, int32_t hi) { return v >= lo && v <= hi; };
    // (gemm_t64, side_stream, chain_wide and spmm_alias are read as thresholds / flags: any value is served)
    if (!in(t->row_chain, 0, 1) /* 2, 3: the executor's backward chains, removed */ || !in(t->attn_impl, 0, 4) || t->attn16_min_lq < 1 || !in(t->f32_split, 0, 7) || t->wgrad_wgs < 1 ||
        !in(t->wgrad_group, 0, 15) || !in(t->wgrad_group_splitk, 0, 8) || t->wgrad_group_wgs < 1 || !in(t->wgrad_group_tail, 0, 1) ||
        !in(t->feats_bf16, 0, 1) || !in(t->ln_fuse, 0, 31) || (t->ln_fuse & 3) /* bit 0: the executor's fused data gradient + LayerNorm backward, bit 1: the 128-row backward panels, removed */ ||
        !in(t->samp_epilogue, 0, 1) || !in(t->gemm_epilogue, 0, 3) ||
        !(in(t->attn16_short, 0, 1) || t->attn16_short == 4 || t->attn16_short == 8) || !in(t->attn16_block, 0, 1)) return ORTK_EINVAL;
    ortk::g_tuning = *t;
    return 0;
}

// ------------------------------------------------------------------------------------------------ dynamic LDS attribute
namespace ortk {
// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (device, function): set once per pair, from any host thread
// (a process-wide `static bool` per call site left the second device of a process without it, and raced)
int lds_attr(const void* fn, size_t bytes) {
    struct Key { int dev; const void* fn; size_t bytes; };
    static std::mutex mu;
    static std::vector<Key>* seen = new std::vector<Key>();
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return ORTK_EINVAL;
    std::lock_guard<std::mutex> lk(mu);
    for (const Key& k : *seen) if (k.dev == dev && k.fn == fn && k.bytes >= bytes) return 0;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return ORTK_EINVAL;
    seen->push_back(Key{dev, fn, bytes});
    return 0;
}
}  // namespace ortk

// ------------------------------------------------------------------------------------------------ profiling hook
// Opt-in, measurement only (bench.py's roofline leg): HIP events around a launch on its stream, accumulated per key (ortk_gemm:
// precision * 4 + transA * 2 + transB; the other launchers: ortk_internal.h PROF_KEY_*).  Disabled by default; the timed region of
// bench.py never runs with it on.
namespace {
struct ProfRec { hipEvent_t a, b; int key; double flops, bytes; int slot; double per_count; double units; };
constexpr int PROF_SLOTS = 1 << 16;
unsigned long long* g_prof_slots = nullptr;      // device counters (ortk::prof_slot)
int g_prof_slot_next = 0;
bool g_prof_on = false;
bool g_prof_serial = false;    // level 1: the executor keeps every launch on the caller's stream (kernels timed in isolation)
std::mutex g_prof_mu;          // decode chunks may be driven by several host threads
std::vector<ProfRec>* g_prof = nullptr;
}  // namespace

namespace ortk {
bool ortk_prof_active() { return g_prof_on; }
bool ortk_prof_serial() { return g_prof_serial; }
// begin records the first event, end the second; a launch whose events cannot be created is simply not recorded
bool prof_begin(int key, double flops, double bytes, hipStream_t s, ProfMark& m) {
    m.live = false;
    if (!g_prof_on) return false;
    if (hipEventCreate(&m.a) != hipSuccess) return false;
    if (hipEventCreate(&m.b) != hipSuccess) { (void)hipEventDestroy(m.a); return false; }
    m.key = key; m.flops = flops; m.bytes = bytes; m.live = true;
    (void)hipEventRecord(m.a, s);
    return true;
}
void prof_end(const ProfMark& m, hipStream_t s) {
    if (!m.live) return;
    (void)hipEventRecord(m.b, s);
    ProfRec rec{m.a, m.b, m.key, m.flops, m.bytes, m.slot, m.per_count, m.units};
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof->push_back(rec);
}
unsigned long long* prof_slot(int* index) {
    if (index) *index = -1;
    if (!g_prof_on || !g_prof_slots || !index) return nullptr;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (g_prof_slot_next >= PROF_SLOTS) return nullptr;
    *index = g_prof_slot_next++;
    return g_prof_slots + *index;
}
}  // namespace ortk

extern "C" int ortk_prof_enable(int32_t on) {
    if (!g_prof) g_prof = new std::vector<ProfRec>();
    for (auto& r : *g_prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    g_prof->clear();
    if (on && !g_prof_slots && hipMalloc(reinterpret_cast<void**>(&g_prof_slots), PROF_SLOTS * sizeof(unsigned long long)) != hipSuccess) g_prof_slots = nullptr;
    if (on && g_prof_slots && hipMemset(g_prof_slots, 0, PROF_SLOTS * sizeof(unsigned long long)) != hipSuccess) return ORTK_EINVAL;
    g_prof_slot_next = 0;
    g_prof_on = on != 0;
    g_prof_serial = on == 1;
    return 0;
}
// Waits for the recorded events (host sync: measurement only).
extern "C" int ortk_prof_collect(int32_t key, int64_t* launches, double* total_ms, double* total_flops) {
    if (!g_prof || !launches || !total_ms || !total_flops) return ORTK_EINVAL;
    *launches = 0; *total_ms = 0; *total_flops = 0;
    for (auto& r : *g_prof) {
        if (r.key != key) continue;
        if (hipEventSynchronize(r.b) != hipSuccess) return ORTK_EINVAL;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) return ORTK_EINVAL;
        *launches += 1; *total_ms += ms; *total_flops += r.flops;
    }
    return 0;
}

// sum over the launches of `key` of the workgroups each one started (recorded by the launchers that size their grids themselves:
// the grouped weight gradients) — launches / this = the average share of the chip such a launch holds
extern "C" int ortk_prof_collect_units(int32_t key, double* total_workgroups) {
    if (!g_prof || !total_workgroups) return ORTK_EINVAL;
    *total_workgroups = 0;
    for (auto& r : *g_prof) if (r.key == key) *total_workgroups += r.units;
    return 0;
}

extern "C" int ortk_prof_collect_bytes(int32_t key, double* total_bytes) {
    if (!g_prof || !total_bytes) return ORTK_EINVAL;
    *total_bytes = 0;
    // (the counters of the slots: the caller has synchronised — ortk_prof_collect waits for every event — and this copy waits as well)
    std::vector<unsigned long long> slots;
    if (g_prof_slots && g_prof_slot_next > 0) {
        slots.resize((size_t)g_prof_slot_next);
        if (hipMemcpy(slots.data(), g_prof_slots, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return ORTK_EINVAL;
    }
    for (auto& r : *g_prof) {
        if (r.key != key) continue;
        *total_bytes += r.bytes;
        if (r.slot >= 0 && (size_t)r.slot < slots.size()) *total_bytes += r.per_count * (double)slots[(size_t)r.slot];
    }
    return 0;
}
