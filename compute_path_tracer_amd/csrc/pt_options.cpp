// pt_options.cpp -- pt_set_option / pt_get_option (include/pt_abi.h): one table
// of the keys, each with how it is set and how it is read.
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

#include "pt_ctx.h"

namespace {

struct Option {
    const char *key;    // a key ending in '_' matches as a prefix (tap_stat_<k>)
    // settable: a value in [lo, hi] goes to *field(c) (else `refusal`), then `set` runs, if any
    int *(*field)(pt_ctx *);
    int lo, hi;
    const char *refusal;
    int (*set)(pt_ctx *, int);  // (without a field: the whole of setting the key)
    // readable: `get`, or the field itself when read_field
    int (*get)(pt_ctx *, const char *key, double *);
    bool read_field;
};

#define FIELD(member) [](pt_ctx *c) -> int * { return &c->member; }
// a plain integer option, set and read
#define OPT_INT(key, member, lo, hi, refusal) {key, FIELD(member), lo, hi, refusal, nullptr, nullptr, true}
// a reading that is a call: int(expr) is its result (`key_`, `v`: the getter's arguments)
#define OPT_GET(key, expr) \
    {key, nullptr, 0, 0, nullptr, nullptr, [](pt_ctx *c, const char *key_, double *v) { (void)key_; return int(expr); }, false}
// ... or one expression of the context `c`
#define OPT_READ(key, expr) OPT_GET(key, (*v = double(expr), PT_OK))

int set_jit(pt_ctx *c, int value) {
    if (!value) pt_jit_disable(c->jit);  // re-enabled on the next pt_set_data
    return PT_OK;
}

int set_jit_wait(pt_ctx *c, int) {  // block until a pending tier-up build is installed
    HIPCHK(c, hipSetDevice(c->device));
    pt_jit_poll(c->jit, true);
    return PT_OK;
}

// "moments" (DESIGN.md 3.28): switching it on allocates and zeroes the moment image, switching it off drops
// the moments' validity (the buffer is kept for the next time); setting the value it has changes nothing
int set_moments(pt_ctx *c, int value) {
    if (value < 0 || value > 1) return fail(c, PT_ERR_INVALID, "moments must be 0 or 1");
    if ((value != 0) == (c->mom.on != 0)) return PT_OK;
    c->mom.on = value ? 1 : 0;
    HIPCHK(c, hipSetDevice(c->device));
    return pt_moments_reset(c);
}

// Waves per SIMD the scene kernel in use can hold: 8 = the 8-wave build
// (<= 64 VGPRs), 7 = the rebuild after a spill (pt_jit_compile_source)
double jit_waves(pt_ctx *c, PtJitStage stage, int threads) {
    const PtJitModule *m = pt_jit_active(c->jit);
    const hipFunction_t f = m ? pt_jit_select(*m, stage, false, false, true, false) : nullptr;
    int blocks = 0;
    if (f && hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, f, threads, 0) != hipSuccess) blocks = 0;
    return double(blocks) * (threads / 64) / 4.0;  // (4 SIMDs per CU)
}

// The table of check[] sets (-1: not in use): bin_sets, the distinct sets the
// last chunk of the last dispatch claimed slots for; bin_overflow, the
// lookups of the last instrumented dispatch (pt_dispatch_stats) whose set
// found no slot within PT_BIN_PROBES and shared its hash bin (pt_binned.h
// bin_resolve)
int read_btab(pt_ctx *c, bool sets, double *value) {
    *value = -1.0;
    if (!(sets ? c->bin.btab_used : c->bin.btab_counted) || !c->bin.btab.p) return PT_OK;
    std::vector<unsigned long long> t(PT_BINS + 1);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(t.data(), c->bin.btab.p, t.size() * sizeof(t[0]), hipMemcpyDeviceToHost));
    if (sets) *value = double(std::count_if(t.begin(), t.end() - 1, [](unsigned long long v) { return v != 0ull; }));
    else *value = double(t.back());
    return PT_OK;
}

// sync: the section's stream was not synchronised after it (pt_render_guides
// and the filter's kernels are asynchronous; pt_display waited for its own)
int section_ms(pt_ctx *c, const TimedSection &t, bool sync, double *v) {
    float ms = 0.0f;
    HIPCHK(c, t.ms(&ms, sync));
    *v = ms;
    return PT_OK;
}

// the stages of the last pt_mesh_extract, summed
int mesh_ms(pt_ctx *c, double *v) {
    *v = 0.0;
    for (const TimedSection &t : c->mesh.stage_time) {
        double ms = 0.0;
        const int rc = section_ms(c, t, false, &ms);
        if (rc != PT_OK) return rc;
        *v += ms;
    }
    return PT_OK;
}

// summed over the dispatch's trace / shade / sky passes
int log_ms(pt_ctx *c, EventLog &g, double *v) {
    HIPCHK(c, g.ms(v));
    return PT_OK;
}

// tap_stat_<k>: counter k of the last stats run's shade-pass taps
int tap_stat(pt_ctx *c, const char *key, double *v) {
    const int k = std::atoi(key + std::strlen("tap_stat_"));
    if (k < 0 || k >= PT_ST_COUNT) return fail(c, PT_ERR_INVALID, "tap_stat index out of range");
    *v = double(c->prog.tap_stats[k]);
    return PT_OK;
}

const Option kOptions[] = {
    OPT_INT("kernel", kernel, PT_KERNEL_AUTO, PT_KERNEL_BINNED, "bad kernel id"),
    OPT_INT("shade_batch", shade_batch, 1, 64, "shade_batch must be in [1, 64]"),
    OPT_INT("bin_lanes", bin.lanes, 1, BinState::kMaxLanes, "bin_lanes must be in [1, 4]"),
    OPT_INT("bin_table", bin.table, 0, 1, "bin_table must be 0 or 1"),
    OPT_INT("shade_taps", bin.shade_taps, 0, 1, "shade_taps must be 0 or 1"),
    OPT_INT("denoise_lds", dn.lds, 0, 1, "denoise_lds must be 0 or 1"),
    OPT_INT("mesh_skip", mesh.skip, 0, 1, "mesh_skip must be 0 or 1"),
    // samples in flight per chunk of a pt_trace_radiance call: at least one ray of PT_RADIANCE_MAX_SPP samples
    OPT_INT("radiance_samples", rad.samples, PT_RADIANCE_MAX_SPP, 1 << 28, "radiance_samples must be in [65536, 2^28]"),
    // set through its own setter (the moment image comes and goes with it), read as it is
    {"moments", nullptr, 0, 0, nullptr, set_moments,
     [](pt_ctx *c, const char *, double *v) { return int((*v = double(c->mom.on), PT_OK)); }, false},
    // set only
    {"jit", FIELD(jit.enabled), 0, 1, "jit must be 0 or 1", set_jit, nullptr, false},
    {"jit_bake", FIELD(jit.bake), 0, 2, "jit_bake must be 0, 1 or 2", nullptr, nullptr, false},  // (at the next pt_set_data)
    {"jit_wait", nullptr, 0, 0, nullptr, set_jit_wait, nullptr, false},
    // set as given, read as the chunk size in use (the automatic one while unset)
    {"bin_samples", FIELD(bin.samples), 64, INT_MAX, "bin_samples must be >= 64", nullptr,
     [](pt_ctx *c, const char *, double *v) { return int((*v = double(pt_bin_samples(c)), PT_OK)); }, false},
    // read only
    OPT_READ("jit_active", pt_jit_active(c->jit) ? 1.0 : 0.0),
    OPT_READ("jit_tier_active", c->jit.tier.module ? 1.0 : 0.0),
    // what pt_set_data derived from the values (pt_derive.cpp): the map() bound's margin (NaN: no bound), and
    // whether every box coordinate is inside bounds()' reciprocal guard
    OPT_READ("bound_k", c->prog.bound_k),
    OPT_READ("fast_bounds", c->prog.fast_bounds ? 1.0 : 0.0),
    OPT_READ("jit_tier_seconds", c->jit.tier_seconds),
    OPT_READ("jit_seconds", c->jit.seconds),
    OPT_READ("jit_trace_waves", jit_waves(c, PtJitStage::Trace, 64)),
    OPT_READ("jit_shade_waves", jit_waves(c, PtJitStage::Shade, PT_BIN_BLOCK)),
    // where the scene kernel in use came from: 1 the shipped on-disk cache
    // (lib/jitcache), 0 this process's hipRTC, -1 none loaded
    OPT_READ("jit_cache", c->jit.tier.module ? c->jit.tier_from : (c->jit.mod.module ? c->jit.from : -1)),
    // the probe modules this context compiled (one per distinct generated source) and their compile seconds
    OPT_READ("probe_compiles", c->probe.compiles),
    OPT_READ("probe_seconds", c->probe.seconds),
    OPT_READ("bin_chunks", c->bin.last_chunks),  // of the last timed binned dispatch
    OPT_READ("bin_fallback", c->bin.fallback ? 1.0 : 0.0),
    OPT_READ("bin_bytes", pt_bin_bytes_held(c)),  // (as allocated: the wide buffers stay once a scene needed them)
    OPT_GET("bin_sets", read_btab(c, true, v)),
    OPT_GET("bin_overflow", read_btab(c, false, v)),
    OPT_READ("gen_trace", c->bin.gen_trace_used),
    OPT_READ("gen_norec", c->bin.gen_norec_used),
    OPT_READ("trace_launches", c->bin.tlog.used / 2),
    OPT_READ("shade_launches", c->bin.slog.used / 2),
    OPT_READ("sky_launches", c->bin.klog.used / 2),
    OPT_GET("trace_ms", log_ms(c, c->bin.tlog, v)),
    OPT_GET("shade_ms", log_ms(c, c->bin.slog, v)),
    OPT_GET("sky_ms", log_ms(c, c->bin.klog, v)),
    OPT_GET("display_ms", section_ms(c, c->img.display_time, false, v)),
    OPT_GET("guide_ms", section_ms(c, c->dn.guide_time, true, v)),
    OPT_GET("denoise_ms", section_ms(c, c->dn.denoise_time, true, v)),
    // the last pt_sample_field's kernel; the last pt_mesh_extract's kernels by stage (the extract waited for them)
    OPT_GET("sample_ms", section_ms(c, c->mesh.sample_time, false, v)),
    OPT_GET("mesh_skip_ms", section_ms(c, c->mesh.stage_time[pt_ctx::Mesher::kSkip], false, v)),
    OPT_GET("mesh_classify_ms", section_ms(c, c->mesh.stage_time[pt_ctx::Mesher::kClassify], false, v)),
    OPT_GET("mesh_scan_ms", section_ms(c, c->mesh.stage_time[pt_ctx::Mesher::kScan], false, v)),
    OPT_GET("mesh_emit_ms", section_ms(c, c->mesh.stage_time[pt_ctx::Mesher::kEmit], false, v)),
    OPT_GET("mesh_ms", mesh_ms(c, v)),
    // the last pt_trace_rays' / pt_pick_pixels' kernel (both calls waited for it)
    OPT_GET("rays_ms", section_ms(c, c->rays.rays_time, false, v)),
    OPT_GET("pick_ms", section_ms(c, c->rays.pick_time, false, v)),
    // the last pt_trace_radiance's kernels, summed over its chunks (the call waited for them), and the shared
    // first segments' part of that (0 in hemisphere mode); the device memory its staging holds
    OPT_GET("radiance_ms", log_ms(c, c->rad.klog, v)),
    OPT_GET("radiance_first_ms", log_ms(c, c->rad.flog, v)),
    OPT_READ("radiance_bytes", c->rad.bytes()),
    // the last pt_render_preview's kernel, without its display pass (the call waited for it)
    OPT_GET("preview_ms", section_ms(c, c->preview.time, false, v)),
    OPT_READ("guides_valid", c->dn.guides_valid ? 1.0 : 0.0),
    // second moments: whether the moment image and the accumulation image are one render's, and of how many frames;
    // the last variance kernel, and all iterations of the last pt_denoise_guided (without its variance and display passes)
    OPT_READ("moments_valid", c->mom.valid ? 1.0 : 0.0),
    OPT_READ("moment_frames", c->mom.valid ? c->mom.frames : 0u),
    OPT_GET("variance_ms", section_ms(c, c->mom.variance_time, true, v)),
    OPT_GET("guided_ms", section_ms(c, c->mom.guided_time, true, v)),
    // temporal accumulation: whether the context holds a history, and of how many accumulates; the last
    // pt_temporal_accumulate's kernel; the last pt_denoise_history's variance kernel and all its iterations
    OPT_READ("history_valid", c->hist.valid ? 1.0 : 0.0),
    OPT_READ("history_views", c->hist.views),
    OPT_GET("temporal_ms", section_ms(c, c->hist.accumulate_time, true, v)),
    OPT_GET("history_variance_ms", section_ms(c, c->hist.variance_time, true, v)),
    OPT_GET("history_denoise_ms", section_ms(c, c->hist.denoise_time, true, v)),
    OPT_GET("tap_stat_", tap_stat(c, key_, v)),
};

const Option *find_option(const char *key) {
    for (const Option &o : kOptions) {
        const size_t n = std::strlen(o.key);
        if (o.key[n - 1] == '_' ? !std::strncmp(key, o.key, n) : !std::strcmp(key, o.key)) return &o;
    }
    return nullptr;
}

}  // namespace

extern "C" int pt_set_option(pt_ctx *c, const char *key, int value) {
    if (!c || !key) return PT_ERR_INVALID;
    const Option *o = find_option(key);
    if (!o || !(o->field || o->set)) return fail(c, PT_ERR_INVALID, std::string("unknown option ") + key);
    if (o->field) {
        if (value < o->lo || value > o->hi) return fail(c, PT_ERR_INVALID, o->refusal);
        *o->field(c) = value;
    }
    return o->set ? o->set(c, value) : PT_OK;
}

extern "C" int pt_get_option(pt_ctx *c, const char *key, double *value) {
    if (!c || !key || !value) return PT_ERR_INVALID;
    const Option *o = find_option(key);
    if (!o || !(o->get || o->read_field)) return fail(c, PT_ERR_INVALID, std::string("unknown option ") + key);
    if (o->get) return o->get(c, key, value);
    *value = double(*o->field(c));
    return PT_OK;
}
