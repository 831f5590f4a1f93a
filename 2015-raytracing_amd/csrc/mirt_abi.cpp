// mirt_abi.cpp -- implementation of include/mirt.h: contexts, buffers, the WebCL-shaped
// kernel objects (argument marshalling + launch validation) and the fused pass.
//
// Everything a launch will touch is checked on the host BEFORE the kernel is enqueued:
// buffer extents against the work-item count, cell-offset tables for monotonicity and
// extent, argument sizes.  A bad argument therefore comes back as an error code; it does
// not become an out-of-bounds access on the GPU.
#include "../../include/mirt.h"
#include "pt_launch.hpp"
#include "pt_post_check.hpp"
#include "pt_rows_plan.hpp"
#include "pt_view_plan.hpp"
#include "pt_set_guard.hpp"
#include "pt_box_exit.hpp"
#include "pt_shadow_gap.hpp"
#include "pt_stream_match.hpp"
#include "pt_upsample_taps.hpp"

#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <atomic>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace {

constexpr size_t kRayBytes = 48, kPoiBytes = 64, kAcuBytes = 16;

thread_local std::string t_last_error = "";

// Live handles, by address AND kind: a handle of the wrong type (a kernel passed where a buffer is expected, a stale address that
// `new` has since handed to another kind of object) fails validation instead of being dereferenced as something it is not.
enum HandleKind : uint8_t { H_CTX = 1, H_BUF, H_KERNEL, H_GRAPH, H_GROUP };
std::mutex g_live_mu;
std::unordered_map<const void*, HandleKind> g_live;
std::atomic<uint64_t> g_next_uid{1};

void live_add(const void* p, HandleKind k) { std::lock_guard<std::mutex> l(g_live_mu); g_live[p] = k; }
void live_del(const void* p) { std::lock_guard<std::mutex> l(g_live_mu); g_live.erase(p); }
bool live_is(const void* p, HandleKind k) {
    if (!p) return false;
    std::lock_guard<std::mutex> l(g_live_mu);
    auto it = g_live.find(p);
    return it != g_live.end() && it->second == k;
}

// The bit mask of an optimistic / exact pair, an allocation of the context: [count, cursor, pad, pad | mask words...].  The optimistic kernel sets
// the bit of what it hands over, the exact kernel walks the bits on the device, and the counter is taken from them when it is asked for.
struct DeferMask {
    void* ptr = nullptr;
    size_t bytes = 0;
    uint32_t words = 0;   // mask words the last call used (0: it ran the exact kernel only, or queued nothing)
    uint32_t unit = 1;    // what a bit stands for in the counter: 1 sample, ray or pixel, or 256 where a bit is a block of 256 samples
    static size_t bytes_for(uint32_t words) { return 16 + (size_t)words * 4; }
    uint32_t* counters() const { return (uint32_t*)ptr; }
    uint32_t* bits() const { return (uint32_t*)ptr + 4; }
};

}  // namespace

struct mirt_graph;
struct mirt_group;

// the kernel table and the stream recogniser: pt_stream_match.hpp (a kernel's named argument indices stay in their namespace: pt::sphereTrace::pois)
using pt::ArgType; using pt::A_BUF; using pt::KernelId; using pt::KernelSpec; using pt::KArg; using pt::Enqueue; using pt::kKernels; using pt::arg_size; using pt::f2u_host;

struct mirt_ctx {
    int device = -1;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string last_error;
    void* scratch = nullptr;  // lens draws of the rpp==1 mode
    size_t scratch_bytes = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // One mask per family of calls, because the counter of one call survives calls of every other kind (mirt_pass_deferred after a mirt_render_ao is
    // still the pass's): the pass (a bit per sample, or per block of 256 where it resolves its own pixels), the guides of both cameras (a bit per pixel;
    // no counter), mirt_trace_closest / mirt_trace_occluded (per ray), mirt_render_ao (per pixel), mirt_trace_radiance (per ray), mirt_render_view (per
    // block of 256 rays) and mirt_view_ao (per pixel).
    DeferMask pass_mask, guide_mask, ray_mask, ao_mask, rad_mask, view_mask, view_ao_mask;
    // The camera table of the batch calls (mirt_view_rays_batch, mirt_render_view_batch): ONE device allocation, filled on the stream by launches
    // whose ARGUMENTS carry the cameras (pt_launch.hpp launch_viewCameras) -- the host array is read while the call runs, and a call queued behind
    // a running one overwrites the table only after that one's kernels.  A call with more frames than the table holds waits for the stream once,
    // frees it and allocates twice the need (upload_cameras); every other call waits for nothing.
    void* camera_table = nullptr;
    size_t camera_table_bytes = 0;
    bool inpass_resolve = true;   // a pass writes pixel / radiance itself where it can (MIRT_INPASS_RESOLVE=0: always the separate copyToPixel)
    bool last_pass_resolved = false;   // render_pass_impl: the pass just queued resolved its own pixels
    int force_exact = 0;          // mirt_ctx_set_exact_only: 1 = skip the optimistic kernel, run every sample through the exact one
    bool profiling = false;       // per-kernel events inside mirt_render_pass
    hipEvent_t pe[3] = {nullptr, nullptr, nullptr};
    bool pe_valid = false;
    bool capturing = false;       // between mirt_capture_begin and mirt_capture_end: the stream records, nothing may wait on it
    // objects created on this context; mirt_ctx_destroy reaps what the host did not release (the reference host leaks its
    // bouncePaths kernel: A10 code.js:1444-1455 never pushes it on cl_resources)
    std::unordered_set<mirt_buf*> bufs;
    std::unordered_set<mirt_kernel*> kernels;
    std::unordered_set<mirt_graph*> graphs;
    mirt_group* group = nullptr;  // set when the context belongs to a device group (mirt_group_create)
    // command-stream fusion (mirt_ctx_set_fusion): enqueues of the Assign10 pass kernels held back until the pass is complete
    int fusion = 0;
    std::vector<Enqueue> pending;
    uint64_t fused_passes = 0;    // passes executed as ONE fused launch because their enqueue stream matched executeRender's
    uint64_t guided_passes = 0;   // mirt_render_first_pass_guided / mirt_render_passes_guided calls whose launch wrote the guides itself (the one-launch route)
    uint64_t guided_views = 0;    // the same for mirt_render_view_guided
    // the same for the frame dialects (mirt_ctx_set_frame_fusion): an A04 / A07 initTrace and the enqueues behind it are held in `pending` too
    bool frame_fusion = false;
    uint64_t fused_frames = 0;
    // what a recording has touched so far (mirt_graph pins): device allocations a replay will read or write
    uint64_t scratch_gen = 1, defer_gen = 1;   // bumped whenever the allocation is replaced
    struct Pin { mirt_buf* buf; uint64_t uid; uint64_t prep_gen; uint64_t version; bool content; };
    std::vector<Pin> cap_pins;
    bool cap_scratch = false, cap_defer = false;
};

// held-back enqueues (command-stream fusion, below): every entry point that observes or changes device state runs them first
static int flush_pending(mirt_ctx* ctx);
#define FLUSH_PENDING(ctx) do { if (!(ctx)->pending.empty()) { int _rc = flush_pending(ctx); if (_rc) return _rc; } } while (0)

struct mirt_graph {
    mirt_ctx* ctx = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    // every allocation the recording captured a raw pointer of; mirt_graph_launch refuses to replay once one of them is gone
    std::vector<mirt_ctx::Pin> pins;
    uint64_t scratch_gen = 0, defer_gen = 0;   // 0: not used by the recording
};

struct mirt_buf {
    mirt_ctx* ctx = nullptr;
    void* ptr = nullptr;
    size_t bytes = 0;
    bool owned = true;
    unsigned flags = 0;
    uint64_t uid = 0;      // unique per allocation: tells a live handle from a new object at a recycled address
    uint64_t version = 1;  // bumped by every host write / device zero / mirt_buf_invalidate
    // cell-offset validation cache
    uint64_t off_version = 0;
    uint32_t off_n = 0;
    uint32_t off_last = 0;
    uint32_t prep_count = 0;   // records in `prep` (the group spheres sit at record index prep_count)
    // prepared-triangle copy of a position buffer (fused path), rebuilt when the contents change
    void* prep = nullptr;
    size_t prep_bytes = 0;
    uint64_t prep_version = 0;
    uint64_t prep_gen = 1;    // bumped whenever `prep` is freed or replaced
    bool prep_sane = false;   // every plane-normal component is 0 or in [2^-40, 2^40]
    bool gap_planes_ok = false;   // `gap_planes` holds the axis planes of the prepared copy's plane list (at most kLdsTriMax records)
    pt::GapPlanes gap_planes;     // read back once per buffer content (ensure_prepared); fill_grid makes a set's plane-free gap from it (pt_shadow_gap.hpp)
};

struct mirt_kernel {
    mirt_ctx* ctx = nullptr;
    const KernelSpec* spec = nullptr;
    std::vector<KArg> args;
};

namespace {

bool live_has(const mirt_ctx* p) { return live_is(p, H_CTX); }
bool live_has(const mirt_buf* p) { return live_is(p, H_BUF); }
bool live_has(const mirt_kernel* p) { return live_is(p, H_KERNEL); }
bool live_has(const mirt_graph* p) { return live_is(p, H_GRAPH); }

int fail(mirt_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    t_last_error = buf;
    if (ctx && live_has(ctx)) ctx->last_error = buf;
    return code;
}

#define HIPCHK(ctx, expr)                                                                          \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return fail((ctx), MIRT_E_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// operations that wait on the stream or move host memory cannot be part of a recording
#define NOT_WHILE_CAPTURING(ctx, what) \
    do { if ((ctx)->capturing) return fail((ctx), MIRT_E_ARG, "%s is not possible inside mirt_capture_begin/end: run the sequence once before recording it", (what)); } while (0)

// The prologue of an entry point that works on the stream and cannot be recorded: a live context, the held-back enqueues run, no recording open.
#define ENTRY_PROLOGUE(ctx, fn)                                                                    \
    do {                                                                                           \
        if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "%s: unknown context", (fn));      \
        FLUSH_PENDING(ctx);                                                                        \
        NOT_WHILE_CAPTURING(ctx, (fn));                                                            \
    } while (0)

// A recording captures raw device pointers.  Every buffer a recorded launch touches is pinned: (handle, allocation uid), plus --
// `content` -- the version of its contents and the generation of its prepared copy when the launch relies on host-side
// validation or preparation of those contents (cell-offset tables, triangle positions).
void pin(mirt_ctx* ctx, const mirt_buf* b, bool content) {
    if (!ctx->capturing) return;
    for (auto& p : ctx->cap_pins)
        if (p.buf == b) { p.content = p.content || content; return; }
    ctx->cap_pins.push_back({const_cast<mirt_buf*>(b), b->uid, b->prep_gen, b->version, content});
}

int need(mirt_ctx* ctx, const char* what, const mirt_buf* b, uint64_t bytes) {
    if (!live_has(b)) return fail(ctx, MIRT_E_HANDLE, "%s: released or unknown buffer", what);
    if (b->ctx != ctx) return fail(ctx, MIRT_E_ARG, "%s: buffer belongs to another context", what);
    if ((uint64_t)b->bytes < bytes)
        return fail(ctx, MIRT_E_RANGE, "%s: buffer holds %zu bytes, launch needs %llu", what, b->bytes, (unsigned long long)bytes);
    pin(ctx, b, false);
    return MIRT_OK;
}

// The same with the label "fn label" (the bare label where fn is nullptr), put together only when the check fails: a successful call formats and
// allocates nothing.
int need(mirt_ctx* ctx, const char* fn, const char* label, const mirt_buf* b, uint64_t bytes) {
    if (live_has(b) && b->ctx == ctx && (uint64_t)b->bytes >= bytes) { pin(ctx, b, false); return MIRT_OK; }
    return need(ctx, fn ? (std::string(fn) + " " + label).c_str() : label, b, bytes);
}

// Checks a cell-offset table (uint[n^3+1], non-decreasing) and that the primitive arrays hold
// off[n^3] entries.  The table is read back once per (buffer contents, n) and cached.
int check_grid(mirt_ctx* ctx, const char* what, mirt_buf* off, uint32_t n, const mirt_buf* prims, size_t prim_stride,
               const mirt_buf* normals, const mirt_buf* matid) {
    if (n == 0 || n > 1024) return fail(ctx, MIRT_E_ARG, "%s: n_slabs %u outside 1..1024", what, n);
    const uint64_t cells = (uint64_t)n * n * n;
    int rc = need(ctx, what, off, (cells + 1) * 4);
    if (rc) return rc;
    // memory the caller owns (mirt_buf_wrap) can change behind the runtime's back: its verdict is never cached
    if (!off->owned || !(off->off_version == off->version && off->off_n == n)) {
        NOT_WHILE_CAPTURING(ctx, "validating a new cell-offset table");
        std::vector<uint32_t> h(cells + 1);
        HIPCHK(ctx, hipMemcpyAsync(h.data(), off->ptr, (cells + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        for (uint64_t i = 0; i < cells; ++i) {
            if (h[i] > h[i + 1]) return fail(ctx, MIRT_E_DATA, "%s: cell offsets decrease at cell %llu", what, (unsigned long long)i);
            if (n > 1 && h[i + 1] - h[i] >= pt::kMaxCellSlots)
                return fail(ctx, MIRT_E_RANGE, "%s: cell %llu holds %u slots (a cell of a grid holds at most %u)", what, (unsigned long long)i, h[i + 1] - h[i], pt::kMaxCellSlots - 1u);
        }
        off->off_version = off->version;
        off->off_n = n;
        off->off_last = h[cells];
    }
    pin(ctx, off, true);
    const uint64_t count = off->off_last;
    rc = need(ctx, what, prims, count * prim_stride);
    if (rc) return rc;
    if (normals && (rc = need(ctx, what, normals, count * prim_stride))) return rc;
    if (matid && (rc = need(ctx, what, matid, count * 4))) return rc;
    return MIRT_OK;
}

int ensure_scratch(mirt_ctx* ctx, size_t bytes);

// (re)builds the prepared-triangle copy of a position buffer when its contents changed
int ensure_prepared(mirt_ctx* ctx, mirt_buf* pb, uint32_t count) {
    // [count records of 48 B][one bounding sphere (float4) per group of records]: the spheres sit right behind the records, so a prepared copy is
    // good for exactly the count it was made for
    const size_t bytes = pt::prepared_bytes(count);
    if (pb->owned && pb->prep_version == pb->version && pb->prep_count == count && pb->prep_bytes >= bytes && (pb->prep || !bytes)) { pin(ctx, pb, true); return MIRT_OK; }
    NOT_WHILE_CAPTURING(ctx, "preparing a new triangle buffer");
    if (pb->prep && pb->prep_bytes < bytes) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(pb->prep)); pb->prep = nullptr; pb->prep_bytes = 0; pb->prep_gen++; }
    if (bytes && !pb->prep) { HIPCHK(ctx, hipMalloc(&pb->prep, bytes)); pb->prep_bytes = bytes; pb->prep_gen++; }
    int rc = ensure_scratch(ctx, 16);
    if (rc) return rc;
    uint32_t insane = 0;
    HIPCHK(ctx, hipMemsetAsync(ctx->scratch, 0, 4, ctx->stream));
    pt::launch_prepTriangles(ctx->stream, pb->ptr, pb->prep, count, (uint32_t*)ctx->scratch);
    HIPCHK(ctx, hipMemcpyAsync(&insane, ctx->scratch, 4, hipMemcpyDeviceToHost, ctx->stream));
    // the plane list of a small set, once per buffer content: the host takes the axis planes from it (pt_shadow_gap.hpp)
    std::vector<uint32_t> planes;
    if (count && count <= pt::kLdsTriMax) {
        planes.resize(pt::prepared_planes_bytes(count) / 4);
        HIPCHK(ctx, hipMemcpyAsync(planes.data(), (const char*)pb->prep + pt::prepared_planes_offset(count), planes.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    pb->prep_sane = insane == 0;
    pb->gap_planes_ok = !planes.empty() && pt::gap_planes_from_list(planes.data(), (uint32_t)planes.size(), count, &pb->gap_planes) != 0;
    pb->prep_version = pb->version;
    if (pb->prep_count != count) pb->prep_gen++;   // rebuilt in place for another count: the group spheres and the sweep array moved, a recorded graph must not replay against it
    pb->prep_count = count;
    return MIRT_OK;
}

int ensure_scratch(mirt_ctx* ctx, size_t bytes) {
    if (ctx->capturing) ctx->cap_scratch = true;
    if (ctx->scratch_bytes >= bytes) return MIRT_OK;
    NOT_WHILE_CAPTURING(ctx, "growing the scratch buffer");
    if (ctx->scratch) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(ctx->scratch)); ctx->scratch = nullptr; ctx->scratch_bytes = 0; }
    ctx->scratch_gen++;
    HIPCHK(ctx, hipMalloc(&ctx->scratch, bytes));
    ctx->scratch_bytes = bytes;
    return MIRT_OK;
}

// A mask grown to its header and `words` mask words where it is smaller, and those bytes cleared on the stream, ahead of the pair.
int grow_and_clear(mirt_ctx* ctx, DeferMask& m, uint32_t words) {
    const size_t need_bytes = DeferMask::bytes_for(words);
    if (m.bytes < need_bytes) {
        if (m.ptr) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(m.ptr)); m.ptr = nullptr; m.bytes = 0; }
        HIPCHK(ctx, hipMalloc(&m.ptr, need_bytes));
        m.bytes = need_bytes;
    }
    HIPCHK(ctx, hipMemsetAsync(m.ptr, 0, need_bytes, ctx->stream));
    return MIRT_OK;
}

// Whether a call runs the optimistic / exact pair: the optimistic kernels are built, the context does not force the exact one, and every set of
// the call passes the geometry-side guard (pt_set_guard.hpp).
bool optimistic(const mirt_ctx* ctx, const pt::FusedArgs& A) { return pt::fused_fast_available() && !ctx->force_exact && pt::all_sets_fast_ok(A); }

// The launches of a call that is one launch: launch(optimistic, mask_out, mask_in).  The pair -- the optimistic kernel writing the cleared mask, then
// the exact kernel over its bits, queued without a host round trip -- or the exact kernel alone; `m` remembers what the counter needs.
template <class Launch>
int queue_pair(mirt_ctx* ctx, DeferMask& m, const pt::FusedArgs& A, uint32_t words, uint32_t unit, Launch launch) {
    m.words = 0;
    if (!optimistic(ctx, A)) { launch(false, nullptr, nullptr); return MIRT_OK; }
    if (int rc = grow_and_clear(ctx, m, words)) return rc;
    launch(true, m.bits(), nullptr);
    launch(false, nullptr, m.bits());
    m.words = words;
    m.unit = unit;
    return MIRT_OK;
}

// What the exact kernel redid in the last call on `m`, counted on demand (one small launch and a stream sync): the mask of that call is still in
// place, the next one clears it.
int count_deferred(mirt_ctx* ctx, const char* fn, const DeferMask& m, uint64_t* out) {
    if (!out) return fail(ctx, MIRT_E_ARG, "%s: null output", fn);
    *out = 0;
    if (!m.words) return MIRT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemsetAsync(m.counters(), 0, 16, ctx->stream));
    pt::launch_deferCount(ctx->stream, m.bits(), m.words, m.counters());
    uint32_t count = 0;
    HIPCHK(ctx, hipMemcpyAsync(&count, m.counters(), 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *out = (uint64_t)count * m.unit;
    return MIRT_OK;
}

// The limits of a descriptor's light and mesh arrays (with_lights false: the call reads no light).  arrays: how the message names them.
int check_desc_arrays(mirt_ctx* ctx, const char* fn, const mirt_pass_desc* d, bool with_lights, const char* arrays) {
    if (with_lights && d->n_lights > MIRT_MAX_LIGHTS) return fail(ctx, MIRT_E_ARG, "%s: %u lights > %d (enqueue the kernels one by one instead)", fn, d->n_lights, MIRT_MAX_LIGHTS);
    if (d->n_meshes > MIRT_MAX_MESHES) return fail(ctx, MIRT_E_ARG, "%s: %u meshes > %d (enqueue the kernels one by one instead)", fn, d->n_meshes, MIRT_MAX_MESHES);
    if ((with_lights && d->n_lights && !d->lights) || (d->n_meshes && !d->meshes)) return fail(ctx, MIRT_E_ARG, "%s: null %s array", fn, arrays);
    return MIRT_OK;
}

// The device ranges of a descriptor's geometry, each buffer whole: what an output of a call on it must not meet (pt_post_check.hpp post_alias)
void add_range(std::vector<pt::PostRange>& in, const mirt_buf* b) { if (b && live_has(b)) in.push_back({(uint64_t)(uintptr_t)b->ptr, (uint64_t)b->bytes, true}); }
void add_geometry_ranges(std::vector<pt::PostRange>& in, const mirt_pass_desc* d) {
    const auto add_grid = [&in](const mirt_grid* g) { if (g) { add_range(in, g->prims); add_range(in, g->normals); add_range(in, g->matid); add_range(in, g->cell_offsets); } };
    add_grid(d->spheres); add_grid(d->triangles);
    for (uint32_t m = 0; m < d->n_meshes; ++m) add_grid(&d->meshes[m]);
}

// A buffer of a call: need()'s label, the handle (nullptr: not given), the bytes the call takes of it, and whether it is written.  BUF_IN_WHOLE: an
// input that no output may meet anywhere, not only in the bytes the call reads.
enum BufRole : uint8_t { BUF_OUT, BUF_IN, BUF_IN_WHOLE };
struct CallBuf { const char* label; mirt_buf* buf; uint64_t bytes; BufRole role = BUF_OUT; };

// What a call on a descriptor's geometry checks of its buffers before anything is queued, in this order: every buffer given is live, this context's
// and large enough (need(fn, label)); with_material, d->material holds an entry; then an output is read by nobody and no input is written -- no
// output's bytes meet an input's, the material's or a geometry buffer's (message out_in, "%s" being fn), nor another output's (message outs; a call
// with one output has none).  out_in == nullptr: the call has no aliasing rule.
template <size_t N>
int check_call_buffers(mirt_ctx* ctx, const char* fn, const CallBuf (&b)[N], const mirt_pass_desc* d, bool with_material, const char* out_in, const char* outs) {
    std::vector<pt::PostRange> in;
    pt::PostRange out[N];
    size_t n_out = 0;
    for (const CallBuf& c : b) {
        if (!c.buf) continue;
        if (int rc = need(ctx, fn, c.label, c.buf, c.bytes)) return rc;
        const pt::PostRange r = {(uint64_t)(uintptr_t)c.buf->ptr, c.role == BUF_IN_WHOLE ? (uint64_t)c.buf->bytes : c.bytes, true};
        if (c.role == BUF_OUT) out[n_out++] = r;
        else in.push_back(r);
    }
    if (with_material) {
        if (int rc = need(ctx, "material", d->material, 16)) return rc;
        add_range(in, d->material);
    }
    if (!out_in) return MIRT_OK;
    add_geometry_ranges(in, d);
    const pt::PostAlias alias = pt::post_alias(in.data(), in.size(), out, n_out);
    if (alias == pt::POST_ALIAS_OUTPUT_INPUT) return fail(ctx, MIRT_E_ARG, out_in, fn);
    if (alias == pt::POST_ALIAS_OUTPUTS) return fail(ctx, MIRT_E_ARG, outs, fn);
    return MIRT_OK;
}
// After the launches: their error, and the outputs given have new contents.
int finish_call(mirt_ctx* ctx, const CallBuf* b, size_t n) {
    HIPCHK(ctx, hipGetLastError());
    for (size_t i = 0; i < n; ++i)
        if (b[i].buf && b[i].role == BUF_OUT) b[i].buf->version++;
    return MIRT_OK;
}

// release paths shared by the public entry points and by mirt_ctx_destroy's reaping of leftovers
void free_buf(mirt_buf* buf, bool ctx_alive) {
    mirt_ctx* ctx = buf->ctx;
    live_del(buf);
    if (ctx_alive) {
        ctx->bufs.erase(buf);
        if ((buf->owned && buf->ptr) || buf->prep) {
            (void)hipSetDevice(ctx->device);
            (void)hipStreamSynchronize(ctx->stream);
        }
        if (buf->owned && buf->ptr) (void)hipFree(buf->ptr);
        if (buf->prep) (void)hipFree(buf->prep);
    }
    delete buf;
}
void free_kernel(mirt_kernel* k, bool ctx_alive) {
    live_del(k);
    if (ctx_alive) k->ctx->kernels.erase(k);
    delete k;
}
void free_graph(mirt_graph* g, bool ctx_alive) {
    live_del(g);
    if (ctx_alive) { g->ctx->graphs.erase(g); (void)hipStreamSynchronize(g->ctx->stream); }
    (void)hipGraphExecDestroy(g->exec);
    (void)hipGraphDestroy(g->graph);
    delete g;
}

}  // namespace

// No C++ exception crosses the C boundary (include/mirt.h): every entry point is a function-try-block.
namespace {
int caught(const char* fn, const char* what) noexcept {
    try { return fail(nullptr, MIRT_E_DEVICE, "%s: %s", fn, what); } catch (...) { return MIRT_E_DEVICE; }
}
}  // namespace
#define MIRT_CATCH(fn, ret)                                                         \
    catch (const std::bad_alloc&) { (void)caught(fn, "out of host memory"); ret; }  \
    catch (const std::exception& e) { (void)caught(fn, e.what()); ret; }            \
    catch (...) { (void)caught(fn, "unexpected C++ exception"); ret; }

extern "C" {

const char* mirt_version(void) try { return "mirt 0.2 (gfx950)"; } MIRT_CATCH("mirt_version", return "")

int mirt_device_count(void) try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
} MIRT_CATCH("mirt_device_count", return MIRT_E_DEVICE)

int mirt_device_name(int device, char* out, size_t cap) try {
    if (!out || cap == 0) return fail(nullptr, MIRT_E_ARG, "mirt_device_name: null output");
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, MIRT_E_NODEVICE, "no HIP device %d", device); }
    snprintf(out, cap, "%s (%s, %d CUs)", p.name[0] ? p.name : "AMD Instinct (name not reported)", p.gcnArchName, p.multiProcessorCount);
    return MIRT_OK;
} MIRT_CATCH("mirt_device_name", return MIRT_E_DEVICE)

static int create_ctx(int device, mirt_ctx** out) {
    *out = nullptr;
    int n = mirt_device_count();
    if (n <= 0) return fail(nullptr, MIRT_E_NODEVICE, "no HIP device visible: libmirt needs an MI355X (gfx950); there is no CPU fallback");
    if (device < 0 || device >= n) return fail(nullptr, MIRT_E_ARG, "device %d out of range (0..%d)", device, n - 1);
    hipDeviceProp_t p;
    HIPCHK(nullptr, hipGetDeviceProperties(&p, device));
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, MIRT_E_NODEVICE, "device %d is %s; libmirt carries gfx950 code objects only", device, p.gcnArchName);
    HIPCHK(nullptr, hipSetDevice(device));
    mirt_ctx* c = new mirt_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) { delete c; return fail(nullptr, MIRT_E_DEVICE, "hipStreamCreate failed"); }
    c->stream = c->own_stream;
    if (const char* f = getenv("MIRT_INPASS_RESOLVE")) c->inpass_resolve = atoi(f) != 0;   // A/B and test switch
    if (const char* f = getenv("MIRT_FUSION")) c->fusion = atoi(f) >= 2 ? 2 : 0;   // same as mirt_ctx_set_fusion: for hosts that cannot be edited at all
    if (const char* f = getenv("MIRT_FRAME_FUSION")) c->frame_fusion = atoi(f) != 0;   // same as mirt_ctx_set_frame_fusion
    (void)hipEventCreate(&c->ev0);
    (void)hipEventCreate(&c->ev1);
    for (auto& e : c->pe) (void)hipEventCreate(&e);
    live_add(c, H_CTX);
    *out = c;
    return MIRT_OK;
}

static int destroy_ctx(mirt_ctx* ctx) {
    (void)hipSetDevice(ctx->device);
    if (ctx->capturing) { hipGraph_t g = nullptr; (void)hipStreamEndCapture(ctx->stream, &g); if (g) (void)hipGraphDestroy(g); ctx->capturing = false; }
    (void)flush_pending(ctx);   // held-back enqueues may write wrapped (caller-owned) memory: they still run
    (void)hipStreamSynchronize(ctx->stream);
    // whatever the host never released goes with the context; those handles become MIRT_E_HANDLE
    while (!ctx->graphs.empty()) free_graph(*ctx->graphs.begin(), true);
    while (!ctx->kernels.empty()) free_kernel(*ctx->kernels.begin(), true);
    while (!ctx->bufs.empty()) free_buf(*ctx->bufs.begin(), true);
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    for (DeferMask* m : {&ctx->pass_mask, &ctx->guide_mask, &ctx->ray_mask, &ctx->ao_mask, &ctx->rad_mask, &ctx->view_mask, &ctx->view_ao_mask})
        if (m->ptr) (void)hipFree(m->ptr);
    if (ctx->camera_table) (void)hipFree(ctx->camera_table);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    for (auto& e : ctx->pe) if (e) (void)hipEventDestroy(e);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    live_del(ctx);
    delete ctx;
    return MIRT_OK;
}

int mirt_ctx_create(int device, mirt_ctx** out) try {
    if (!out) return fail(nullptr, MIRT_E_ARG, "mirt_ctx_create: null out");
    return create_ctx(device, out);
} MIRT_CATCH("mirt_ctx_create", return MIRT_E_DEVICE)

int mirt_ctx_destroy(mirt_ctx* ctx) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_ctx_destroy: unknown context");
    if (ctx->group) return fail(ctx, MIRT_E_ARG, "mirt_ctx_destroy: the context belongs to a device group; destroy the group");
    return destroy_ctx(ctx);
} MIRT_CATCH("mirt_ctx_destroy", return MIRT_E_DEVICE)

// ---- device groups: N contexts in one process + the one exchange of the path ---------------------------------------------
// RCCL is bound at run time (dlopen of librccl.so) the first time a group with more than one device -- or a forced RCCL gather --
// is created: a single-GPU host never loads it.
extern "C++" {
namespace {
struct Rccl {
    void* lib = nullptr;
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    std::string err;
};
Rccl& rccl() {
    static Rccl r;
    if (r.lib || !r.err.empty()) return r;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) if ((r.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    if (!r.lib) { r.err = std::string("cannot load librccl.so: ") + (dlerror() ? dlerror() : "?"); return r; }
    auto sym = [&](const char* n) { void* p = dlsym(r.lib, n); if (!p && r.err.empty()) r.err = std::string("librccl.so lacks ") + n; return p; };
    r.CommInitAll = (int (*)(void**, int, const int*))sym("ncclCommInitAll");
    r.CommDestroy = (int (*)(void*))sym("ncclCommDestroy");
    r.GroupStart = (int (*)())sym("ncclGroupStart");
    r.GroupEnd = (int (*)())sym("ncclGroupEnd");
    r.Send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))sym("ncclSend");
    r.Recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))sym("ncclRecv");
    r.GetErrorString = (const char* (*)(int))sym("ncclGetErrorString");
    return r;
}
constexpr int kNcclUint8 = 1;   // ncclUint8 / ncclChar family: rccl.h ncclDataType_t { ncclInt8 = 0, ncclUint8 = 1, ... }
}  // namespace
}  // extern "C++"

struct mirt_group {
    std::vector<mirt_ctx*> ctxs;
    std::vector<void*> comms;    // ncclComm_t per device; empty until a gather needs RCCL
    bool repeated_devices = false;   // rehearsal group (MIRT_GROUP_ALLOW_REPEATED_DEVICES): several contexts on one device
    std::vector<uint8_t> peer;   // [i * n + j]: context i's device reads context j's device's memory directly (hipDeviceEnablePeerAccess succeeded; 1 on the diagonal
                                 // and between contexts that share a device)
    std::vector<int> route;      // per tile, how the last mirt_gather moved it (MIRT_ROUTE_*)
};

static bool live_group(const mirt_group* g) { return live_is(g, H_GROUP); }

static int group_comms(mirt_group* g) {
    if (!g->comms.empty()) return MIRT_OK;
    Rccl& R = rccl();
    if (!R.err.empty()) return fail(g->ctxs[0], MIRT_E_DEVICE, "mirt_gather: %s", R.err.c_str());
    std::vector<int> devs;
    for (auto* c : g->ctxs) devs.push_back(c->device);
    g->comms.assign(devs.size(), nullptr);
    int rc = R.CommInitAll(g->comms.data(), (int)devs.size(), devs.data());
    if (rc != 0) { g->comms.clear(); return fail(g->ctxs[0], MIRT_E_DEVICE, "ncclCommInitAll over %zu devices: %s", devs.size(), R.GetErrorString(rc)); }
    return MIRT_OK;
}

int mirt_group_create(const int* device_ids, int n, mirt_group** out) try {
    if (!out) return fail(nullptr, MIRT_E_ARG, "mirt_group_create: null out");
    *out = nullptr;
    if (!device_ids || n < 1 || n > 64) return fail(nullptr, MIRT_E_ARG, "mirt_group_create: need 1..64 device ids");
    // A device may appear once -- unless MIRT_GROUP_ALLOW_REPEATED_DEVICES=1 (a rehearsal switch: N contexts share the devices at hand, so
    // the whole N-tile path -- tile arithmetic, N fused passes, the gather's offsets and orderings -- runs on a one-GPU box; such a group
    // gathers by device copies, RCCL wants one device per rank)
    bool repeated = false;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (device_ids[i] == device_ids[j]) repeated = true;
    if (repeated) {
        const char* e = getenv("MIRT_GROUP_ALLOW_REPEATED_DEVICES");
        if (!e || atoi(e) != 1) return fail(nullptr, MIRT_E_ARG, "mirt_group_create: a device is listed twice (MIRT_GROUP_ALLOW_REPEATED_DEVICES=1 allows it for rehearsals)");
    }
    mirt_group* g = new mirt_group();
    g->repeated_devices = repeated;
    for (int i = 0; i < n; ++i) {
        mirt_ctx* c = nullptr;
        int rc = create_ctx(device_ids[i], &c);
        if (rc) { for (auto* d : g->ctxs) { d->group = nullptr; destroy_ctx(d); } delete g; return rc; }
        c->group = g;
        g->ctxs.push_back(c);
    }
    // peer access both ways between every pair of distinct devices: what makes hipMemcpyPeerAsync (the copy transport of mirt_gather) a direct xGMI
    // transfer instead of a bounce through host memory.  A pair the runtime refuses stays 0 and its copies are reported as MIRT_ROUTE_STAGED.
    g->peer.assign((size_t)n * n, 0);
    g->route.assign((size_t)n, MIRT_ROUTE_NONE);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const int di = g->ctxs[i]->device, dj = g->ctxs[j]->device;
            if (di == dj) { g->peer[(size_t)i * n + j] = 1; continue; }
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, di, dj) != hipSuccess || !can) { (void)hipGetLastError(); continue; }
            if (hipSetDevice(di) != hipSuccess) { (void)hipGetLastError(); continue; }
            const hipError_t e = hipDeviceEnablePeerAccess(dj, 0);
            if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) g->peer[(size_t)i * n + j] = 1;
            (void)hipGetLastError();
        }
    live_add(g, H_GROUP);
    *out = g;
    return MIRT_OK;
} MIRT_CATCH("mirt_group_create", return MIRT_E_DEVICE)

int mirt_group_peer_access(const mirt_group* g, int i, int j) try {
    if (!live_group(g)) return MIRT_E_HANDLE;
    const int n = (int)g->ctxs.size();
    if (i < 0 || j < 0 || i >= n || j >= n) return MIRT_E_ARG;
    return g->peer[(size_t)i * n + j];
} MIRT_CATCH("mirt_group_peer_access", return MIRT_E_DEVICE)

int mirt_gather_route(const mirt_group* g, int tile) try {
    if (!live_group(g)) return MIRT_E_HANDLE;
    if (tile < 0 || tile >= (int)g->route.size()) return MIRT_E_ARG;
    return g->route[(size_t)tile];
} MIRT_CATCH("mirt_gather_route", return MIRT_E_DEVICE)

int mirt_abi_version(void) { return MIRT_ABI_VERSION; }

int mirt_group_size(const mirt_group* g) try { return live_group(g) ? (int)g->ctxs.size() : MIRT_E_HANDLE; } MIRT_CATCH("mirt_group_size", return MIRT_E_DEVICE)

mirt_ctx* mirt_group_ctx(const mirt_group* g, int index) try {
    if (!live_group(g) || index < 0 || index >= (int)g->ctxs.size()) { fail(nullptr, MIRT_E_ARG, "mirt_group_ctx: unknown group or index out of range"); return nullptr; }
    return g->ctxs[index];
} MIRT_CATCH("mirt_group_ctx", return nullptr)

int mirt_group_destroy(mirt_group* g) try {
    if (!live_group(g)) return fail(nullptr, MIRT_E_HANDLE, "mirt_group_destroy: unknown group");
    for (auto* c : g->ctxs) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); }
    if (!g->comms.empty()) for (void* c : g->comms) if (c) (void)rccl().CommDestroy(c);
    for (size_t i = 0; i < g->ctxs.size(); ++i) {
        g->ctxs[i]->group = nullptr;
        destroy_ctx(g->ctxs[i]);
    }
    live_del(g);
    delete g;
    return MIRT_OK;
} MIRT_CATCH("mirt_group_destroy", return MIRT_E_DEVICE)

void mirt_tile_rows(uint32_t height, uint32_t n_tiles, uint32_t index, uint32_t* row0, uint32_t* nrows) try {
    // contiguous row tiles whose sizes differ by at most one row: the first height % n tiles take the extra row
    if (!n_tiles || index >= n_tiles) { if (row0) *row0 = 0; if (nrows) *nrows = 0; return; }
    const uint32_t q = height / n_tiles, r = height % n_tiles;
    if (row0) *row0 = index * q + (index < r ? index : r);
    if (nrows) *nrows = q + (index < r ? 1u : 0u);
} MIRT_CATCH("mirt_tile_rows", return)

int mirt_gather(mirt_group* g, mirt_buf* const* tiles, const size_t* tile_bytes, int n_tiles, mirt_buf* out, int root, int transport) try {
    if (!live_group(g)) return fail(nullptr, MIRT_E_HANDLE, "mirt_gather: unknown group");
    const int n = (int)g->ctxs.size();
    mirt_ctx* rc_ctx = g->ctxs[0];
    // arguments first: nothing is flushed or queued on any device for a call that is going to be refused
    if (!tiles || !tile_bytes || root < 0 || root >= n) return fail(rc_ctx, MIRT_E_ARG, "mirt_gather: null argument or root out of range");
    if (n_tiles != n) return fail(rc_ctx, MIRT_E_ARG, "mirt_gather: %d tiles for a group of %d contexts", n_tiles, n);
    if (transport != MIRT_GATHER_AUTO && transport != MIRT_GATHER_RCCL && transport != MIRT_GATHER_COPY)
        return fail(rc_ctx, MIRT_E_ARG, "mirt_gather: transport %d is not MIRT_GATHER_AUTO / _RCCL / _COPY", transport);
    mirt_ctx* rootc = g->ctxs[root];
    uint64_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (!live_has(tiles[i]) || tiles[i]->ctx != g->ctxs[i]) return fail(rc_ctx, MIRT_E_HANDLE, "mirt_gather: tile %d is not a live buffer of the group's context %d", i, i);
        if (tiles[i]->bytes < tile_bytes[i]) return fail(rc_ctx, MIRT_E_RANGE, "mirt_gather: tile %d holds %zu bytes, asked to send %zu", i, tiles[i]->bytes, tile_bytes[i]);
        total += tile_bytes[i];
    }
    if (!live_has(out) || out->ctx != rootc) return fail(rc_ctx, MIRT_E_HANDLE, "mirt_gather: the output is not a live buffer of the root context");
    if (out->bytes < total) return fail(rc_ctx, MIRT_E_RANGE, "mirt_gather: output holds %zu bytes, the tiles add up to %llu", out->bytes, (unsigned long long)total);
    for (auto* c : g->ctxs) NOT_WHILE_CAPTURING(c, "mirt_gather");
    for (auto* c : g->ctxs) FLUSH_PENDING(c);
    // MIRT_GATHER_AUTO: RCCL when the group spans several distinct devices and librccl loads, else copies
    bool use_rccl = transport == MIRT_GATHER_RCCL;
    if (transport == MIRT_GATHER_AUTO && n > 1 && !g->repeated_devices) use_rccl = rccl().err.empty();
    if (use_rccl && g->repeated_devices) return fail(rc_ctx, MIRT_E_ARG, "mirt_gather: RCCL needs one device per context (this group lists a device twice: MIRT_GATHER_COPY)");
    if (!use_rccl) {
        // copies queued on the root's stream, each ordered after the work queued so far on the tile's own stream: tile == frame for one
        // context; device-to-device across contexts that share a device; hipMemcpyPeerAsync (xGMI, P2P) across devices
        HIPCHK(rootc, hipSetDevice(rootc->device));
        uint64_t off = 0;
        for (int i = 0; i < n; ++i) {
            mirt_ctx* c = g->ctxs[i];
            if (tile_bytes[i]) {
                if (c->stream != rootc->stream) {
                    hipEvent_t ev;
                    HIPCHK(rootc, hipSetDevice(c->device));
                    HIPCHK(rootc, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
                    hipError_t e = hipEventRecord(ev, c->stream);
                    if (e == hipSuccess) { (void)hipSetDevice(rootc->device); e = hipStreamWaitEvent(rootc->stream, ev, 0); }
                    (void)hipEventDestroy(ev);   // released once the wait has been satisfied
                    HIPCHK(rootc, hipSetDevice(rootc->device));
                    HIPCHK(rootc, e);
                }
                if (c->device == rootc->device) HIPCHK(rootc, hipMemcpyAsync((char*)out->ptr + off, tiles[i]->ptr, tile_bytes[i], hipMemcpyDeviceToDevice, rootc->stream));
                else HIPCHK(rootc, hipMemcpyPeerAsync((char*)out->ptr + off, rootc->device, tiles[i]->ptr, c->device, tile_bytes[i], rootc->stream));
                g->route[(size_t)i] = c->device == rootc->device ? MIRT_ROUTE_LOCAL : (g->peer[(size_t)root * n + i] ? MIRT_ROUTE_PEER : MIRT_ROUTE_STAGED);
            } else g->route[(size_t)i] = MIRT_ROUTE_NONE;
            off += tile_bytes[i];
        }
        out->version++;
        return MIRT_OK;
    }
    int rc = group_comms(g);
    if (rc) return rc;
    Rccl& R = rccl();
    // one grouped exchange: every device sends its tile to the root (the root's own tile included: a self send/recv pair is legal
    // inside a group), the root receives each at that tile's offset.  N - 1 peers -> N - 1 distinct xGMI links into the root.
    int nrc = R.GroupStart();
    uint64_t off = 0;
    for (int i = 0; i < n && nrc == 0; ++i) {
        if (tile_bytes[i]) {
            (void)hipSetDevice(g->ctxs[i]->device);
            nrc = R.Send(tiles[i]->ptr, tile_bytes[i], kNcclUint8, root, g->comms[i], g->ctxs[i]->stream);
            (void)hipSetDevice(rootc->device);
            if (nrc == 0) nrc = R.Recv((char*)out->ptr + off, tile_bytes[i], kNcclUint8, i, g->comms[root], rootc->stream);
        }
        off += tile_bytes[i];
    }
    const int erc = R.GroupEnd();
    (void)hipSetDevice(rootc->device);
    if (nrc == 0) nrc = erc;
    if (nrc != 0) return fail(rc_ctx, MIRT_E_DEVICE, "mirt_gather: RCCL: %s", R.GetErrorString(nrc));
    for (int i = 0; i < n; ++i) g->route[(size_t)i] = tile_bytes[i] ? MIRT_ROUTE_RCCL : MIRT_ROUTE_NONE;
    out->version++;
    return MIRT_OK;
} MIRT_CATCH("mirt_gather", return MIRT_E_DEVICE)

int mirt_group_finish(mirt_group* g) try {
    if (!live_group(g)) return fail(nullptr, MIRT_E_HANDLE, "mirt_group_finish: unknown group");
    for (auto* c : g->ctxs) {
        NOT_WHILE_CAPTURING(c, "mirt_group_finish");
        FLUSH_PENDING(c);
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return MIRT_OK;
} MIRT_CATCH("mirt_group_finish", return MIRT_E_DEVICE)

const char* mirt_last_error(mirt_ctx* ctx) try {
    if (ctx && live_has(ctx)) return ctx->last_error.c_str();
    return t_last_error.c_str();
} MIRT_CATCH("mirt_last_error", return "")

int mirt_ctx_set_stream(mirt_ctx* ctx, void* hip_stream) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_ctx_set_stream: unknown context");
    NOT_WHILE_CAPTURING(ctx, "mirt_ctx_set_stream");
    FLUSH_PENDING(ctx);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return MIRT_OK;
} MIRT_CATCH("mirt_ctx_set_stream", return MIRT_E_DEVICE)

int mirt_finish(mirt_ctx* ctx) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_finish: unknown context");
    NOT_WHILE_CAPTURING(ctx, "mirt_finish");
    // inside a held pass (the reference calls finish() after every sceneRender, A10 code.js:1406) nothing is observable until a read, which
    // flushes -- unless the pass works on memory the caller can reach behind the ABI (mirt_buf_wrap): then finish() means finish
    if (!ctx->pending.empty() && pt::is_frame_init(ctx->pending[0].spec->id)) FLUSH_PENDING(ctx);   // a held frame runs at finish (the pages read the pixels next)
    if (ctx->fusion >= 2 && !ctx->pending.empty()) {
        bool wrapped = false;
        for (const auto& p : ctx->pending)
            for (size_t j = 0; j < p.args.size(); ++j)
                if (p.spec->args[j] == A_BUF && live_has(p.args[j].buf) && !p.args[j].buf->owned) wrapped = true;
        if (!wrapped) return MIRT_OK;
        FLUSH_PENDING(ctx);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MIRT_OK;
} MIRT_CATCH("mirt_finish", return MIRT_E_DEVICE)

int mirt_buf_create(mirt_ctx* ctx, size_t bytes, unsigned flags, mirt_buf** out) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_buf_create: unknown context");
    if (!out) return fail(ctx, MIRT_E_ARG, "mirt_buf_create: null out");
    *out = nullptr;
    if (bytes == 0) return fail(ctx, MIRT_E_ARG, "mirt_buf_create: zero-size buffer (WebCL INVALID_BUFFER_SIZE)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    void* p = nullptr;
    HIPCHK(ctx, hipMalloc(&p, bytes));
    mirt_buf* b = new mirt_buf();
    b->ctx = ctx; b->ptr = p; b->bytes = bytes; b->owned = true; b->flags = flags; b->uid = g_next_uid++;
    live_add(b, H_BUF);
    ctx->bufs.insert(b);
    *out = b;
    return MIRT_OK;
} MIRT_CATCH("mirt_buf_create", return MIRT_E_DEVICE)

int mirt_buf_wrap(mirt_ctx* ctx, void* device_ptr, size_t bytes, mirt_buf** out) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_buf_wrap: unknown context");
    if (!out || !device_ptr || bytes == 0) return fail(ctx, MIRT_E_ARG, "mirt_buf_wrap: null pointer or zero size");
    if (((uintptr_t)device_ptr & 15u) != 0) return fail(ctx, MIRT_E_ARG, "mirt_buf_wrap: device pointer must be 16-byte aligned");
    mirt_buf* b = new mirt_buf();
    b->ctx = ctx; b->ptr = device_ptr; b->bytes = bytes; b->owned = false; b->flags = MIRT_MEM_READ_WRITE; b->uid = g_next_uid++;
    live_add(b, H_BUF);
    ctx->bufs.insert(b);
    *out = b;
    return MIRT_OK;
} MIRT_CATCH("mirt_buf_wrap", return MIRT_E_DEVICE)

int mirt_buf_release(mirt_buf* buf) try {
    if (!live_has(buf)) return fail(nullptr, MIRT_E_HANDLE, "mirt_buf_release: unknown or already released buffer");
    if (live_has(buf->ctx)) { mirt_ctx* ctx = buf->ctx; FLUSH_PENDING(ctx); }
    free_buf(buf, live_has(buf->ctx));
    return MIRT_OK;
} MIRT_CATCH("mirt_buf_release", return MIRT_E_DEVICE)

int mirt_buf_invalidate(mirt_buf* buf) try {
    if (!live_has(buf)) return fail(nullptr, MIRT_E_HANDLE, "mirt_buf_invalidate: unknown buffer");
    buf->version++;
    return MIRT_OK;
} MIRT_CATCH("mirt_buf_invalidate", return MIRT_E_DEVICE)

size_t mirt_buf_size(const mirt_buf* buf) try { return live_has(buf) ? buf->bytes : 0; } MIRT_CATCH("mirt_buf_size", return 0)
void* mirt_buf_device_ptr(const mirt_buf* buf) try {
    if (!live_has(buf)) return nullptr;
    if (live_has(buf->ctx)) (void)flush_pending(buf->ctx);   // the caller is about to look at the memory itself
    return buf->ptr;
} MIRT_CATCH("mirt_buf_device_ptr", return nullptr)

int mirt_buf_write(mirt_buf* buf, size_t offset, size_t nbytes, const void* host, int blocking) try {
    (void)blocking;
    if (!live_has(buf)) return fail(nullptr, MIRT_E_HANDLE, "mirt_buf_write: unknown buffer");
    mirt_ctx* ctx = buf->ctx;
    NOT_WHILE_CAPTURING(ctx, "mirt_buf_write");
    FLUSH_PENDING(ctx);
    if (!host && nbytes) return fail(ctx, MIRT_E_ARG, "mirt_buf_write: null host pointer");
    if (offset > buf->bytes || nbytes > buf->bytes - offset)
        return fail(ctx, MIRT_E_RANGE, "mirt_buf_write: [%zu, +%zu) exceeds buffer of %zu bytes", offset, nbytes, buf->bytes);
    if (!nbytes) return MIRT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync((char*)buf->ptr + offset, host, nbytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the host array is borrowed for this call only
    buf->version++;
    return MIRT_OK;
} MIRT_CATCH("mirt_buf_write", return MIRT_E_DEVICE)

int mirt_buf_read(mirt_buf* buf, size_t offset, size_t nbytes, void* host, int blocking) try {
    (void)blocking;
    if (!live_has(buf)) return fail(nullptr, MIRT_E_HANDLE, "mirt_buf_read: unknown buffer");
    mirt_ctx* ctx = buf->ctx;
    NOT_WHILE_CAPTURING(ctx, "mirt_buf_read");
    FLUSH_PENDING(ctx);
    if (!host && nbytes) return fail(ctx, MIRT_E_ARG, "mirt_buf_read: null host pointer");
    if (offset > buf->bytes || nbytes > buf->bytes - offset)
        return fail(ctx, MIRT_E_RANGE, "mirt_buf_read: [%zu, +%zu) exceeds buffer of %zu bytes", offset, nbytes, buf->bytes);
    if (!nbytes) return MIRT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(host, (const char*)buf->ptr + offset, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MIRT_OK;
} MIRT_CATCH("mirt_buf_read", return MIRT_E_DEVICE)

// OpenCL C text with comments blanked out, and the names of its `__kernel void NAME(` definitions
static void scan_source(const char* source, std::string* code, std::vector<std::string>* kernels) {
    const char* p = source;
    while (*p) {
        if (p[0] == '/' && p[1] == '*') { p += 2; while (*p && !(p[0] == '*' && p[1] == '/')) ++p; if (*p) p += 2; code->push_back(' '); continue; }
        if (p[0] == '/' && p[1] == '/') { while (*p && *p != '\n') ++p; continue; }
        code->push_back(*p++);
    }
    size_t pos = 0;
    while ((pos = code->find("__kernel", pos)) != std::string::npos) {
        size_t q = pos + 8;
        auto ws = [&](size_t i) { while (i < code->size() && strchr(" \t\r\n", (*code)[i])) ++i; return i; };
        q = ws(q);
        if (code->compare(q, 4, "void") == 0) {
            q = ws(q + 4);
            size_t e = q;
            while (e < code->size() && (isalnum((unsigned char)(*code)[e]) || (*code)[e] == '_')) ++e;
            if (e > q) kernels->push_back(code->substr(q, e - q));
        }
        pos += 8;
    }
}

int mirt_program_dialect(const char* source) try {
    if (!source) return 0;
    std::string code;
    std::vector<std::string> ks;
    scan_source(source, &code, &ks);
    auto has = [&](const char* k) { for (auto& n : ks) if (n == k) return true; return false; };
    auto text = [&](const char* t) { return code.find(t) != std::string::npos; };
    if (has("bouncePaths") && has("sceneRender")) return 10;
    if (has("sceneRender") || has("initShadowTrace")) return 0;      // A08 / A09: earlier drafts of the A10 set, not built
    if (has("meshTrace")) {
        if (text("z_stride")) return 7;                              // 3-D grid (A07 code.cl:545)
        if (!text("n_slabs") && !text("AABB bound")) return 4;       // brute force, no pre-clip (A04)
        return 0;                                                    // A05 / A06: not built
    }
    if (ks.size() == 1 && ks[0] == "raytrace" && !text("__global float4")) return 1;   // A02's raytrace takes atom arrays
    return 0;
} MIRT_CATCH("mirt_program_dialect", return MIRT_E_DEVICE)

int mirt_program_check(mirt_ctx* ctx, const char* source, char* missing, size_t cap) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_program_check: unknown context");
    if (!source) return fail(ctx, MIRT_E_ARG, "mirt_program_check: null source");
    std::string code, miss;
    std::vector<std::string> ks;
    scan_source(source, &code, &ks);
    const int dialect = mirt_program_dialect(source);
    const std::string prefix = dialect == 7 ? "A07:" : dialect == 4 ? "A04:" : dialect == 1 ? "A01:" : "";
    int n_missing = 0;
    for (const auto& name : ks) {
        bool found = false;
        for (const auto& k : kKernels) if (prefix + name == k.name) found = true;
        if (!found) { if (n_missing++) miss += ","; miss += name; }
    }
    if (missing && cap) snprintf(missing, cap, "%s", miss.c_str());
    return n_missing;
} MIRT_CATCH("mirt_program_check", return MIRT_E_DEVICE)

int mirt_kernel_get(mirt_ctx* ctx, const char* name, mirt_kernel** out) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_kernel_get: unknown context");
    if (!name || !out) return fail(ctx, MIRT_E_ARG, "mirt_kernel_get: null argument");
    *out = nullptr;
    for (const auto& s : kKernels) {
        if (strcmp(name, s.name) == 0) {
            mirt_kernel* k = new mirt_kernel();
            k->ctx = ctx; k->spec = &s; k->args.resize(s.args.size());
            live_add(k, H_KERNEL);
            ctx->kernels.insert(k);
            *out = k;
            return MIRT_OK;
        }
    }
    return fail(ctx, MIRT_E_NAME, "no kernel named '%s' (INVALID_KERNEL_NAME)", name);
} MIRT_CATCH("mirt_kernel_get", return MIRT_E_DEVICE)

int mirt_kernel_release(mirt_kernel* k) try {
    if (!live_has(k)) return fail(nullptr, MIRT_E_HANDLE, "mirt_kernel_release: unknown or already released kernel");
    free_kernel(k, live_has(k->ctx));
    return MIRT_OK;
} MIRT_CATCH("mirt_kernel_release", return MIRT_E_DEVICE)

int mirt_kernel_num_args(const mirt_kernel* k) try { return live_has(k) ? (int)k->spec->args.size() : MIRT_E_HANDLE; } MIRT_CATCH("mirt_kernel_num_args", return MIRT_E_DEVICE)
int mirt_kernel_preferred_multiple(const mirt_kernel* k) try { return live_has(k) ? 64 : MIRT_E_HANDLE; } MIRT_CATCH("mirt_kernel_preferred_multiple", return MIRT_E_DEVICE)

int mirt_kernel_set_arg(mirt_kernel* k, unsigned index, size_t size, const void* value) try {
    if (!live_has(k)) return fail(nullptr, MIRT_E_HANDLE, "mirt_kernel_set_arg: unknown kernel");
    mirt_ctx* ctx = k->ctx;
    if (index >= k->args.size()) return fail(ctx, MIRT_E_ARG, "%s: argument index %u out of range (%zu args)", k->spec->name, index, k->args.size());
    ArgType t = k->spec->args[index];
    if (t == A_BUF) return fail(ctx, MIRT_E_ARG, "%s: argument %u is a buffer; use mirt_kernel_set_arg_buf", k->spec->name, index);
    if (!value || size != arg_size(t))
        return fail(ctx, MIRT_E_ARG, "%s: argument %u expects %zu bytes, got %zu (INVALID_ARG_SIZE)", k->spec->name, index, arg_size(t), size);
    memcpy(&k->args[index].val, value, size);
    k->args[index].set = true;
    return MIRT_OK;
} MIRT_CATCH("mirt_kernel_set_arg", return MIRT_E_DEVICE)

int mirt_kernel_set_arg_buf(mirt_kernel* k, unsigned index, mirt_buf* buf) try {
    if (!live_has(k)) return fail(nullptr, MIRT_E_HANDLE, "mirt_kernel_set_arg_buf: unknown kernel");
    mirt_ctx* ctx = k->ctx;
    if (index >= k->args.size()) return fail(ctx, MIRT_E_ARG, "%s: argument index %u out of range", k->spec->name, index);
    if (k->spec->args[index] != A_BUF) return fail(ctx, MIRT_E_ARG, "%s: argument %u is not a buffer", k->spec->name, index);
    if (!live_has(buf)) return fail(ctx, MIRT_E_HANDLE, "%s: argument %u: unknown or released buffer", k->spec->name, index);
    if (buf->ctx != ctx) return fail(ctx, MIRT_E_ARG, "%s: argument %u: buffer belongs to another context", k->spec->name, index);
    k->args[index].buf = buf;
    k->args[index].set = true;
    return MIRT_OK;
} MIRT_CATCH("mirt_kernel_set_arg_buf", return MIRT_E_DEVICE)

// ---- command-stream fusion ---------------------------------------------------------------------------------------------------
// The reference host issues one pass as 44+ enqueues (A10 code.js:1806-1854), every stage round-tripping Ray / Poi / shadow Ray / acu
// through HBM: 4.2 KB per sample against the fused pass's 24 B.  With mirt_ctx_set_fusion(ctx, 2) the runtime holds the enqueues of
// the Assign10 pass kernels back, and when the stream from an initTrace up to a copyToPixel IS executeRender's sequence over one
// consistent set of buffers -- initTrace, the closest-hit kernels, lightRender per light, per light {initShadowTrace, any-hit kernels,
// sceneRender}, any number of {bouncePaths, closest-hit kernels, per-light block}, copyToPixel -- it runs the pass as ONE launch of
// k_fusedPass (render_pass_impl) + the recorded copyToPixel.  Anything else (a different order, mixed buffers, a read / write / release /
// other command in between) flushes the held enqueues one by one, unchanged.  See include/mirt.h for what the mode trades.
// How render_pass_impl runs a pass.  passes > 1: that many progressive passes in one launch (mirt_render_passes), pass_index the first of them.
// mark_start false: the profiling interval goes on from the event an earlier pass of the same mirt_render_passes call recorded.
// MIRT_PASSES_EVERY_FRAME: `every` -- the launch resolves in the kernel and writes all `passes` frames (pt_launch.hpp FusedArgs::every) -- or
// `frame`: an ordinary pass writes frame slot `frame` of pixel / radiance.
struct PassOpts {
    bool fresh = false;
    uint32_t passes = 1;
    bool mark_start = true;
    uint32_t frame = 0;
    bool every = false;
    mirt_buf* guide_nh = nullptr;   // mirt_render_first_pass_guided, mirt_render_passes_guided: the first-hit guides of the tile are written too (either may be null)
    mirt_buf* guide_ad = nullptr;
    // which rule sends them to the pass's own launch (pt_pass_plan.hpp): the first-pass call's, or mirt_render_passes_guided's for its one-launch
    // routes.  That call's ordinary-passes route runs the guides' checks with its first pass (GUIDES_CHECK_ONLY: nothing of them is queued) and
    // queues the guide launches behind its last (GUIDES_BEHIND).
    enum GuideMode { GUIDES_FIRST_PASS, GUIDES_PASSES, GUIDES_BEHIND, GUIDES_CHECK_ONLY } guide_mode = GUIDES_FIRST_PASS;
    const char* guide_fn = "mirt_render_first_pass_guided";   // the entry point its messages name
    float tone = NAN;   // try_fuse_pass: the tone factor of the recorded copyToPixel, as the host passed it (one pass).  NaN: computed from the pass index
};
static int render_pass_impl(mirt_ctx* ctx, const mirt_pass_desc* d, const PassOpts& o);
static int launch_kernel(mirt_ctx* ctx, const KernelSpec& S, std::vector<KArg>& a, unsigned dim, const size_t* global);
static int render_frame_impl(mirt_ctx* ctx, const mirt_frame_desc* d, uint32_t aa = 1u);

// The frame dialects' counterpart of try_fuse_pass.  MIRT_OK: the held stream was a frame (match_frame, pt_stream_match.hpp) and ran as one launch; the
// ray buffer is not written.  1: not a frame, or refused before anything was launched (nothing executed).  < 0: error.
static int try_fuse_frame(mirt_ctx* ctx, const std::vector<Enqueue>& P) {
    pt::FrameMatch m;
    if (!pt::match_frame(P, &m)) return 1;
    mirt_frame_desc d;
    memset(&d, 0, sizeof d);
    d.struct_size = sizeof d;
    d.assign = m.assign; d.width = m.width; d.height = m.height;
    memcpy(d.cam, m.cam, 64);
    memcpy(d.bounds, m.bounds, 32);
    d.n_slabs = m.n_slabs;
    if (m.mesh) { d.t_size = m.t_size; d.t_pos = m.t_pos; d.t_normal = m.t_normal; d.t_mindex = m.t_mindex; d.t_mcolor = m.t_mcolor; d.t_slab_size = m.t_slab_size; }
    if (m.mol) { d.s_size = m.s_size; d.s_atoms = m.s_atoms; d.s_mindex = m.s_mindex; d.s_mcolor = m.s_mcolor; d.s_slab_size = m.s_slab_size; }
    d.pixel = m.pixels;
    // the kernels check the ray buffer's extent too: a stream whose rays are too small fails enqueue by enqueue, as issued
    if (!live_has(m.rays) || (uint64_t)m.rays->bytes < (uint64_t)m.width * m.height * kRayBytes) return 1;
    const int rc = render_frame_impl(ctx, &d);
    if (rc && rc != MIRT_E_DEVICE) return 1;
    if (rc) return rc;
    ctx->fused_frames++;
    return MIRT_OK;
}

// MIRT_OK: the held stream was a whole pass (match_pass, pt_stream_match.hpp) and has been executed fused.  1: not a pass (nothing executed).  < 0: error.
static int try_fuse_pass(mirt_ctx* ctx, const std::vector<Enqueue>& P) {
    pt::PassMatch m;
    if (!pt::match_pass(P, &m)) return 1;
    // ---- it is a pass: one fused launch + the recorded copyToPixel
    mirt_pass_desc d;
    memset(&d, 0, sizeof d);
    d.struct_size = sizeof d;
    d.width = m.width; d.height = m.height; d.rays_per_pixel = m.rpp; d.bounces = m.bounces; d.pass_index = 1;
    memcpy(d.cam, m.cam, 64);
    memcpy(d.scene_bounds, m.scene_bounds, 32);
    d.focal_length = m.focal_length; d.lens_rad = m.lens_rad;
    size_t k = 0;
    if (m.spheres) d.spheres = &m.sets[k++];
    if (m.triangles) d.triangles = &m.sets[k++];
    d.meshes = k < m.sets.size() ? &m.sets[k] : nullptr;
    d.n_meshes = (uint32_t)(m.sets.size() - k);
    d.lights = m.lights.data(); d.n_lights = (uint32_t)m.lights.size();
    d.material = m.material; d.seeds = m.seeds; d.acu = m.acu;
    // the recorded copyToPixel goes into the pass where the pass can resolve its own pixels (whole pixels per block of 256 ray ids): its pixel buffer and
    // its factor as the host passed it; where it cannot, render_pass_impl queues the separate kernel behind the pass, with that factor
    d.pixel = m.pixel;
    PassOpts o;
    o.tone = m.tone;
    const int rc = render_pass_impl(ctx, &d, o);
    if (rc && rc != MIRT_E_DEVICE) return 1;   // refused before anything was launched (a size, a grid that fails validation ...): run the stream as issued,
    if (rc) return rc;                          // whose own checks then report it against the kernel that trips it
    m.pixel->version++;   // (written by the pass itself, or by the copyToPixel render_pass_impl queued behind it with the recorded factor)
    ctx->fused_passes++;
    return MIRT_OK;
}

// run whatever is held back: as one fused pass when it is one, else enqueue by enqueue, unchanged
static int flush_pending(mirt_ctx* ctx) {
    if (ctx->pending.empty()) return MIRT_OK;
    std::vector<Enqueue> P;
    P.swap(ctx->pending);
    for (auto& p : P)
        for (size_t j = 0; j < p.args.size(); ++j)
            if (p.spec->args[j] == A_BUF && (!live_has(p.args[j].buf) || p.args[j].buf->ctx != ctx))
                return fail(ctx, MIRT_E_HANDLE, "%s: a buffer of a held-back enqueue was released", p.spec->name);
    int rc = pt::is_frame_init(P[0].spec->id) ? try_fuse_frame(ctx, P) : try_fuse_pass(ctx, P);
    if (rc <= 0) return rc;
    for (auto& p : P)
        if ((rc = launch_kernel(ctx, *p.spec, p.args, p.dim, p.g))) return rc;
    return MIRT_OK;
}

static bool is_pass_kernel(KernelId k) { return k >= pt::K_initTrace && k <= pt::K_copyToPixel; }

int mirt_enqueue(mirt_ctx* ctx, mirt_kernel* k, unsigned dim, const size_t* global, const size_t* local) try {
    (void)local;  // no kernel uses local memory or barriers: the work-group shape is ours to choose
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_enqueue: unknown context");
    if (!live_has(k) || k->ctx != ctx) return fail(ctx, MIRT_E_HANDLE, "mirt_enqueue: unknown kernel");
    const KernelSpec& S = *k->spec;
    if (!global || dim < 1 || dim > 3) return fail(ctx, MIRT_E_ARG, "%s: bad NDRange", S.name);
    for (size_t i = 0; i < k->args.size(); ++i) {
        if (!k->args[i].set) return fail(ctx, MIRT_E_UNSET, "%s: argument %zu was never set (INVALID_KERNEL_ARGS)", S.name, i);
        if (S.args[i] == A_BUF && !live_has(k->args[i].buf)) return fail(ctx, MIRT_E_HANDLE, "%s: argument %zu: buffer was released", S.name, i);
        if (S.args[i] == A_BUF) pin(ctx, k->args[i].buf, false);
    }
    for (unsigned d = 0; d < dim; ++d)
        if (global[d] > 0xFFFFFFFFull) return fail(ctx, MIRT_E_ARG, "%s: global size exceeds 2^32", S.name);
    if (ctx->frame_fusion && !ctx->capturing) {
        // From an A04 / A07 initTrace on EVERY enqueue is held, whatever its kernel: the recogniser judges the stream as the host issued it, so a
        // frame with anything else inside it (a second initTrace, a kernel of another dialect, stages out of order) runs enqueue by enqueue, whole
        const bool held = !ctx->pending.empty() && pt::is_frame_init(ctx->pending[0].spec->id);
        if (held || pt::is_frame_init(S.id)) {
            if (!held) FLUSH_PENDING(ctx);                               // (a held Assign10 pass)
            Enqueue p;
            p.spec = &S; p.args = k->args; p.dim = dim;
            for (unsigned d = 0; d < 3; ++d) p.g[d] = d < dim ? global[d] : 1;
            ctx->pending.push_back(std::move(p));
            if (ctx->pending.size() > 3) return flush_pending(ctx);     // longer than any frame: it is not one, run it now
            return MIRT_OK;
        }
    }
    if (!ctx->pending.empty() && pt::is_frame_init(ctx->pending[0].spec->id)) FLUSH_PENDING(ctx);   // anything else ends a held frame
    if (ctx->fusion >= 2 && !ctx->capturing && is_pass_kernel(S.id)) {
        if (S.id == pt::K_initTrace) FLUSH_PENDING(ctx);                 // a new pass begins: whatever was held is not one
        if (S.id == pt::K_initTrace || !ctx->pending.empty()) {
            Enqueue p;
            p.spec = &S; p.args = k->args; p.dim = dim;
            for (unsigned d = 0; d < 3; ++d) p.g[d] = d < dim ? global[d] : 1;
            ctx->pending.push_back(std::move(p));
            if (S.id == pt::K_copyToPixel) return flush_pending(ctx);    // the pass is complete: run it now
            return MIRT_OK;
        }
    }
    FLUSH_PENDING(ctx);
    return launch_kernel(ctx, S, k->args, dim, global);
} MIRT_CATCH("mirt_enqueue", return MIRT_E_DEVICE)

// The buffer rules of the Assign04 / Assign07 trace stages, for launch_kernel's frame kernels and for render_frame_impl: each checks the stage's buffers
// (`who`: the kernel or the entry point the message names), prepares the triangles the stage reads, and fills the stage's fields of the launch's arguments.
static int frame_a04_mesh(mirt_ctx* ctx, const std::string& who, uint32_t T, mirt_buf* t_pos, const mirt_buf* t_normal, const mirt_buf* t_mindex, const mirt_buf* m_color, pt::FrameArgs& A) {
    if (int rc = need(ctx, (who + " t_pos").c_str(), t_pos, (uint64_t)T * 48)) return rc;
    if (int rc = need(ctx, (who + " t_normal").c_str(), t_normal, (uint64_t)T * 48)) return rc;
    if (int rc = need(ctx, (who + " t_mindex").c_str(), t_mindex, (uint64_t)T * 4)) return rc;
    if (int rc = need(ctx, (who + " m_color").c_str(), m_color, 16)) return rc;
    if (int rc = ensure_prepared(ctx, t_pos, T)) return rc;
    A.t_size = T; A.prep = t_pos->prep; A.normals = t_normal->ptr; A.mindex = t_mindex->ptr; A.mcolor = m_color->ptr; A.ncolors = (uint32_t)(m_color->bytes / 16);
    return MIRT_OK;
}
static int frame_a07_mesh(mirt_ctx* ctx, const std::string& who, const float* bound, uint32_t n_slabs, mirt_buf* slab_size, mirt_buf* t_pos, const mirt_buf* t_normal, pt::FrameArgs& A) {
    if (int rc = check_grid(ctx, (who + " mesh grid").c_str(), slab_size, n_slabs, t_pos, 48, t_normal, nullptr)) return rc;
    if (int rc = ensure_prepared(ctx, t_pos, slab_size->off_last)) return rc;
    memcpy(A.bound, bound, 32); A.n_slabs = n_slabs; A.prep = t_pos->prep; A.normals = t_normal->ptr; A.slab_size = slab_size->ptr; A.n_slots = slab_size->off_last;
    return MIRT_OK;
}
// s_mindex / m_color are bound by the reference host but never read by the kernel (A07 code.cl:459-460)
static int frame_a07_mol(mirt_ctx* ctx, const std::string& who, const float* bound, uint32_t n_slabs, mirt_buf* slab_size, const mirt_buf* s_atoms, pt::FrameArgs& A) {
    if (int rc = check_grid(ctx, (who + " molecule grid").c_str(), slab_size, n_slabs, s_atoms, 16, nullptr, nullptr)) return rc;
    memcpy(A.bound, bound, 32); A.n_slabs = n_slabs; A.atoms = s_atoms->ptr; A.mol_slab_size = slab_size->ptr;
    return MIRT_OK;
}

static int launch_kernel(mirt_ctx* ctx, const KernelSpec& S, std::vector<KArg>& a, unsigned dim, const size_t* global) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t g0 = (uint32_t)global[0];
    int rc;
    auto A = [&](auto j) { return pt::arg(a, j); };   // the argument by its name: a buffer handle, a scalar, or the floats of a float16 / AABB
    switch (S.id) {
        case pt::K_sizeofRay:
        case pt::K_sizeofPoi: {
            namespace K = pt::sizeofRay;
            if ((rc = need(ctx, S.name, A(K::size), 4))) return rc;
            pt::launch_sizeof(st, S.id == pt::K_sizeofRay, (uint32_t*)A(K::size)->ptr);
            break;
        }
        case pt::K_initAcu: {
            namespace K = pt::initAcu;
            uint32_t cnt = std::min(g0, A(K::total));
            if ((rc = need(ctx, S.name, A(K::acu), (uint64_t)cnt * kAcuBytes))) return rc;
            pt::launch_initAcu(st, A(K::acu)->ptr, A(K::total), g0);
            A(K::acu)->version++;
            break;
        }
        case pt::K_initTrace: {
            namespace K = pt::initTrace;
            if (dim != 2) return fail(ctx, MIRT_E_ARG, "initTrace is a 2-D NDRange (A10 code.js:1330)");
            const uint32_t g1 = (uint32_t)global[1];
            const uint32_t cols = f2u_host(A(K::fcam)[14]), rows = f2u_host(A(K::fcam)[15]);
            const uint32_t rpp = A(K::rays_per_pixel);
            const uint32_t wc = std::min(g0, cols), wr = std::min(g1, rows);
            if (wc && wr) {
                if (rpp == 0) return fail(ctx, MIRT_E_ARG, "initTrace: rays_per_pixel is 0");
                uint64_t nrays = ((uint64_t)cols * (wr - 1) + wc) * rpp;  // one past the last ray touched
                if ((rc = need(ctx, "initTrace rays", A(K::rays), nrays * kRayBytes))) return rc;
                if ((rc = need(ctx, "initTrace pois", A(K::pois), nrays * kPoiBytes))) return rc;
                if (rpp == 1) {
                    if ((rc = need(ctx, "initTrace seeds", A(K::seeds), (uint64_t)wc * 4))) return rc;
                    if ((rc = ensure_scratch(ctx, (size_t)cols * rows * 8))) return rc;
                    pt::launch_lensDraws(st, A(K::seeds)->ptr, ctx->scratch, cols, rows, g0, g1, 0, rows);
                }
                pt::launch_initTrace(st, A(K::rays)->ptr, A(K::pois)->ptr, ctx->scratch, A(K::bound), A(K::fcam), A(K::focal_length), A(K::lens_rad), rpp, g0, g1);
            }
            break;
        }
        case pt::K_sphereTrace: {
            namespace K = pt::sphereTrace;
            uint32_t cnt = std::min(g0, A(K::total));
            if ((rc = need(ctx, "sphereTrace pois", A(K::pois), (uint64_t)cnt * kPoiBytes))) return rc;
            if ((rc = need(ctx, "sphereTrace rays", A(K::rays), (uint64_t)cnt * kRayBytes))) return rc;
            if ((rc = check_grid(ctx, "sphereTrace grid", A(K::off), A(K::n_slabs), A(K::prims), 16, nullptr, A(K::matid)))) return rc;
            pt::launch_closest(st, pt::KIND_SPHERES, A(K::total), A(K::pois)->ptr, A(K::rays)->ptr, A(K::prims)->ptr, nullptr, A(K::matid)->ptr, 0, A(K::off)->ptr, A(K::bounds), A(K::n_slabs),
                               pt::set_exit_is_far_face(A(K::bounds), A(K::n_slabs)), g0);
            break;
        }
        case pt::K_triangleTrace: {
            namespace K = pt::triangleTrace;
            uint32_t cnt = std::min(g0, A(K::total));
            if ((rc = need(ctx, "triangleTrace pois", A(K::pois), (uint64_t)cnt * kPoiBytes))) return rc;
            if ((rc = need(ctx, "triangleTrace rays", A(K::rays), (uint64_t)cnt * kRayBytes))) return rc;
            if ((rc = check_grid(ctx, "triangleTrace grid", A(K::off), A(K::n_slabs), A(K::prims), 48, A(K::normals), A(K::matid)))) return rc;
            if ((rc = ensure_prepared(ctx, A(K::prims), A(K::off)->off_last))) return rc;
            pt::launch_closest(st, pt::KIND_TRIANGLES, A(K::total), A(K::pois)->ptr, A(K::rays)->ptr, A(K::prims)->prep, A(K::normals)->ptr, A(K::matid)->ptr, 0, A(K::off)->ptr, A(K::bounds), A(K::n_slabs),
                               pt::set_exit_is_far_face(A(K::bounds), A(K::n_slabs)), g0);
            break;
        }
        case pt::K_meshTrace: {
            namespace K = pt::meshTrace;
            uint32_t cnt = std::min(g0, A(K::total));
            if ((rc = need(ctx, "meshTrace pois", A(K::pois), (uint64_t)cnt * kPoiBytes))) return rc;
            if ((rc = need(ctx, "meshTrace rays", A(K::rays), (uint64_t)cnt * kRayBytes))) return rc;
            if ((rc = check_grid(ctx, "meshTrace grid", A(K::off), A(K::n_slabs), A(K::prims), 48, A(K::normals), nullptr))) return rc;
            if ((rc = ensure_prepared(ctx, A(K::prims), A(K::off)->off_last))) return rc;
            pt::launch_closest(st, pt::KIND_TRIANGLES, A(K::total), A(K::pois)->ptr, A(K::rays)->ptr, A(K::prims)->prep, A(K::normals)->ptr, nullptr, A(K::matid), A(K::off)->ptr, A(K::bounds), A(K::n_slabs),
                               pt::set_exit_is_far_face(A(K::bounds), A(K::n_slabs)), g0);
            break;
        }
        case pt::K_lightRender: {
            namespace K = pt::lightRender;
            uint32_t cnt = std::min(g0, A(K::total));
            if ((rc = need(ctx, "lightRender pois", A(K::pois), (uint64_t)cnt * kPoiBytes))) return rc;
            if ((rc = need(ctx, "lightRender rays", A(K::rays), (uint64_t)cnt * kRayBytes))) return rc;
            if ((rc = need(ctx, "lightRender acu", A(K::acu), (uint64_t)cnt * kAcuBytes))) return rc;
            pt::launch_lightRender(st, A(K::pois)->ptr, A(K::rays)->ptr, A(K::acu)->ptr, A(K::light_info), A(K::total), g0);
            break;
        }
        case pt::K_initShadowTrace: {
            namespace K = pt::initShadowTrace;
            uint32_t cnt = std::min(g0, A(K::total));
            if ((rc = need(ctx, "initShadowTrace shadow", A(K::shadow_rays), (uint64_t)cnt * kRayBytes))) return rc;
            if ((rc = need(ctx, "initShadowTrace pois", A(K::pois), (uint64_t)cnt * kPoiBytes))) return rc;
            if ((rc = need(ctx, "initShadowTrace seeds", A(K::seeds), (uint64_t)cnt * 4))) return rc;
            pt::launch_initShadowTrace(st, A(K::shadow_rays)->ptr, A(K::pois)->ptr, A(K::total), A(K::light_info), A(K::seeds)->ptr, g0);
            break;
        }
        case pt::K_sphereShadowTrace: {
            namespace K = pt::shadowTrace;
            uint32_t cnt = std::min(g0, A(K::total));
            if ((rc = need(ctx, "sphereShadowTrace shadow", A(K::shadow_rays), (uint64_t)cnt * kRayBytes))) return rc;
            if ((rc = check_grid(ctx, "sphereShadowTrace grid", A(K::off), A(K::n_slabs), A(K::prims), 16, nullptr, nullptr))) return rc;
            pt::launch_anyhit(st, pt::KIND_SPHERES, A(K::total), A(K::shadow_rays)->ptr, A(K::prims)->ptr, A(K::off)->ptr, A(K::bounds), A(K::n_slabs), pt::set_exit_is_far_face(A(K::bounds), A(K::n_slabs)), g0);
            break;
        }
        case pt::K_triangleShadowTrace: {
            namespace K = pt::shadowTrace;
            uint32_t cnt = std::min(g0, A(K::total));
            if ((rc = need(ctx, "triangleShadowTrace shadow", A(K::shadow_rays), (uint64_t)cnt * kRayBytes))) return rc;
            if ((rc = check_grid(ctx, "triangleShadowTrace grid", A(K::off), A(K::n_slabs), A(K::prims), 48, nullptr, nullptr))) return rc;
            if ((rc = ensure_prepared(ctx, A(K::prims), A(K::off)->off_last))) return rc;
            pt::launch_anyhit(st, pt::KIND_TRIANGLES, A(K::total), A(K::shadow_rays)->ptr, A(K::prims)->prep, A(K::off)->ptr, A(K::bounds), A(K::n_slabs), pt::set_exit_is_far_face(A(K::bounds), A(K::n_slabs)), g0);
            break;
        }
        case pt::K_sceneRender: {
            namespace K = pt::sceneRender;
            uint32_t cnt = std::min(g0, A(K::total));
            if ((rc = need(ctx, "sceneRender acu", A(K::acu), (uint64_t)cnt * kAcuBytes))) return rc;
            if ((rc = need(ctx, "sceneRender pois", A(K::pois), (uint64_t)cnt * kPoiBytes))) return rc;
            if ((rc = need(ctx, "sceneRender shadow", A(K::shadow_rays), (uint64_t)cnt * kRayBytes))) return rc;
            pt::launch_sceneRender(st, A(K::acu)->ptr, A(K::pois)->ptr, A(K::shadow_rays)->ptr, A(K::material)->ptr, (uint32_t)(A(K::material)->bytes / 16), A(K::light_info), A(K::total), g0);
            break;
        }
        case pt::K_bouncePaths: {
            namespace K = pt::bouncePaths;
            uint32_t cnt = std::min(g0, A(K::total));
            if ((rc = need(ctx, "bouncePaths pois", A(K::pois), (uint64_t)cnt * kPoiBytes))) return rc;
            if ((rc = need(ctx, "bouncePaths rays", A(K::rays), (uint64_t)cnt * kRayBytes))) return rc;
            if ((rc = need(ctx, "bouncePaths seeds", A(K::seeds), (uint64_t)cnt * 4))) return rc;
            pt::launch_bouncePaths(st, A(K::pois)->ptr, A(K::rays)->ptr, A(K::seeds)->ptr, A(K::total), g0);
            break;
        }
        case pt::K_copyToPixel: {
            namespace K = pt::copyToPixel;
            uint32_t cnt = std::min(g0, A(K::pixels));
            if ((rc = need(ctx, "copyToPixel pixel", A(K::pixel), (uint64_t)cnt * 4))) return rc;
            if ((rc = need(ctx, "copyToPixel acu", A(K::acu), (uint64_t)cnt * A(K::rays_per_pixel) * kAcuBytes))) return rc;
            pt::launch_copyToPixel(st, A(K::pixel)->ptr, A(K::acu)->ptr, A(K::m), A(K::pixels), A(K::rays_per_pixel), g0, nullptr);
            break;
        }
        case pt::K_a04_sizeofRay:
        case pt::K_a07_sizeofRay: {
            namespace K = pt::sizeofRay;
            if ((rc = need(ctx, S.name, A(K::size), 4))) return rc;
            pt::launch_sizeof(st, true, (uint32_t*)A(K::size)->ptr);
            break;
        }
        case pt::K_a01_raytrace: {
            namespace K = pt::frame;
            if (dim != 2) return fail(ctx, MIRT_E_ARG, "raytrace is a 2-D NDRange (A01 code.js:241)");
            const uint32_t g1 = (uint32_t)global[1];
            const uint32_t rows = f2u_host(A(K::fcam)[14]), cols = f2u_host(A(K::fcam)[15]);   // A01 packs rows, cols (code.js:50)
            const uint32_t wc = std::min(g0, cols), wr = std::min(g1, rows);
            if (wc && wr) {
                if ((rc = need(ctx, "raytrace pixels", A(K::pixels), ((uint64_t)cols * (wr - 1) + wc) * 4))) return rc;
                pt::launch_a01_raytrace(st, A(K::pixels)->ptr, A(K::fcam), g0, g1);
            }
            break;
        }
        case pt::K_a04_initTrace:
        case pt::K_a07_initTrace:
        case pt::K_a04_meshTrace:
        case pt::K_a07_meshTrace:
        case pt::K_a07_molTrace: {
            namespace K = pt::frame;
            if (dim != 2) return fail(ctx, MIRT_E_ARG, "%s is a 2-D NDRange", S.name);
            const uint32_t g1 = (uint32_t)global[1];
            const uint32_t cols = f2u_host(A(K::fcam)[14]), rows = f2u_host(A(K::fcam)[15]);
            const uint32_t wc = std::min(g0, cols), wr = std::min(g1, rows);
            if (!wc || !wr) break;
            const uint64_t npx = (uint64_t)cols * (wr - 1) + wc;
            if ((rc = need(ctx, "pixels", A(K::pixels), npx * 4))) return rc;
            if ((rc = need(ctx, "rays", A(K::rays), npx * kRayBytes))) return rc;
            if (S.id == pt::K_a04_initTrace) pt::launch_frame_initTrace(st, false, A(K::pixels)->ptr, A(K::fcam), A(K::rays)->ptr, nullptr, g0, g1);
            else if (S.id == pt::K_a07_initTrace) pt::launch_frame_initTrace(st, true, A(K::pixels)->ptr, A(K::fcam), A(K::rays)->ptr, A(pt::a07_initTrace::bound), g0, g1);
            else {
                namespace M4 = pt::a04_meshTrace; namespace MM = pt::a07_molTrace; namespace MT = pt::a07_meshTrace;
                pt::FrameArgs F = {};
                memcpy(F.cam, A(K::fcam), 64); F.pixels = A(K::pixels)->ptr; F.rays = A(K::rays)->ptr; F.gx = g0; F.gy = g1;
                if (S.id == pt::K_a04_meshTrace) rc = frame_a04_mesh(ctx, S.name, A(M4::t_size), A(M4::t_pos), A(M4::t_normal), A(M4::t_mindex), A(M4::m_color), F);
                else if (S.id == pt::K_a07_molTrace) rc = frame_a07_mol(ctx, S.name, A(MM::bound), A(MM::n_slabs), A(MM::slab_size), A(MM::s_atoms), F);
                else rc = frame_a07_mesh(ctx, S.name, A(MT::bound), A(MT::n_slabs), A(MT::slab_size), A(MT::t_pos), A(MT::t_normal), F);
                if (rc) return rc;
                pt::launch_frame_stage(st, F, S.id == pt::K_a04_meshTrace ? pt::FS_A04 : S.id == pt::K_a07_molTrace ? pt::FS_MOL : pt::FS_MESH);
            }
            break;
        }
        default:
            return fail(ctx, MIRT_E_NAME, "kernel not implemented");
    }
    HIPCHK(ctx, hipGetLastError());
    return MIRT_OK;
}

static int fill_grid(mirt_ctx* ctx, const char* what, const mirt_grid* g, bool tri, bool per_prim_matid, pt::GridArgs* o) {
    if (!g->prims || !g->cell_offsets) return fail(ctx, MIRT_E_ARG, "%s: null geometry buffer", what);
    if (tri && !g->normals) return fail(ctx, MIRT_E_ARG, "%s: triangles need a normal buffer", what);
    if (per_prim_matid && !g->matid) return fail(ctx, MIRT_E_ARG, "%s: needs a per-primitive material buffer", what);
    int rc = check_grid(ctx, what, g->cell_offsets, g->n_slabs, g->prims, tri ? 48 : 16, tri ? g->normals : nullptr,
                        per_prim_matid ? g->matid : nullptr);
    if (rc) return rc;
    o->prims = g->prims->ptr;
    o->kind = tri ? pt::KIND_TRIANGLES : pt::KIND_SPHERES;
    if (tri) {
        mirt_buf* pb = g->prims;
        if ((rc = ensure_prepared(ctx, pb, g->cell_offsets->off_last))) return rc;
        o->prims = pb->prep ? pb->prep : pb->ptr;
        o->pnorm = pb->prep && g->cell_offsets->off_last <= pt::kLdsTriMax ? (const char*)pb->prep + pt::prepared_planes_offset(g->cell_offsets->off_last) : nullptr;
    }
    o->normals = tri ? g->normals->ptr : nullptr;
    o->matid = per_prim_matid ? g->matid->ptr : nullptr;
    o->off = g->cell_offsets->ptr;
    memcpy(o->bound, g->bounds, sizeof o->bound);
    o->n = g->n_slabs;
    o->mesh_matid = g->mesh_matid;
    o->nslots = g->cell_offsets->off_last;   // validated by check_grid above
    // the geometry-side guard of the optimistic kernel and the walk's wave-uniform quotients (pt_set_guard.hpp)
    const pt::SetGuard v = pt::set_guard(g->bounds, g->n_slabs, !tri || g->prims->prep_sane);
    o->fast_ok = v.fast_ok;
    o->walk_ok = v.walk_ok;
    o->exit_is_far_face = v.exit_is_far_face;
    o->exit_far_axes = v.exit_far_axes;
    memcpy(o->exit_up, v.exit_up, sizeof o->exit_up);
    // the constant of the one slab pass of a single-cell set (pt_box_exit.hpp; zero where no exit plane lies above its face, and for a grid)
    const pt::BoxExit be = pt::box_exit_consts(g->bounds, v.exit_up);
    o->exit_above_axes = v.exit_above_axes;
    memcpy(&o->exit_gap_max, &be.gap_max, 4);   // (GridArgs holds its bits)
    memcpy(o->delta, v.delta, sizeof o->delta);
    memcpy(o->rdelta, v.rdelta, sizeof o->rdelta);
    // the plane-free gap of a single-cell triangle set with a plane list, for these bounds (pt_shadow_gap.hpp)
    o->gap_ok = 0u;
    memset(o->gap, 0, sizeof o->gap);
    if (tri && o->pnorm && g->n_slabs == 1u && v.fast_ok && g->prims->gap_planes_ok && g->prims->prep_count == g->cell_offsets->off_last) {
        const pt::ShadowGap sg = pt::shadow_gap(g->bounds, v.exit_up, &g->prims->gap_planes, 1.0);
        memcpy(o->gap, sg.qlo, 12); memcpy(o->gap + 3, sg.qhi, 12); memcpy(o->gap + 6, sg.gm, 12); memcpy(o->gap + 9, sg.hm, 12);
        o->gap_ok = sg.ok;
    }
    return MIRT_OK;
}

// what the plan of a pass is asked for (pt_pass_plan.hpp), from the descriptor as the caller gave it
static pt::PassRequest pass_request(const mirt_ctx* ctx, const mirt_pass_desc* d, const PassOpts& o) {
    pt::PassRequest r;
    r.rpp = d->rays_per_pixel;
    r.npix = (uint64_t)(d->nrows ? d->nrows : d->height) * d->width;
    r.passes = o.passes;
    r.fresh = o.fresh;
    r.has_acu = d->acu != nullptr;
    r.has_pixel = d->pixel != nullptr;
    r.has_radiance = d->radiance != nullptr;
    r.every = o.every;
    r.inpass_resolve = ctx->inpass_resolve;
    return r;
}

// What mirt_render_pass and mirt_render_guides check and fill alike, in this order: the descriptor, the k x k ray count, the tile, then the camera,
// bounds, primitive sets (validated and prepared: fill_grid) and material of `A`.  guides: the lights and pass_index are not looked at.
// !with_material (mirt_render_ao, with guides): nor is the material.
static int fill_sets(mirt_ctx* ctx, const char* fn, const mirt_pass_desc* d, pt::FusedArgs& A);
static int fill_shading(mirt_ctx* ctx, const mirt_pass_desc* d, pt::FusedArgs& A, bool with_material);
static int pass_setup(mirt_ctx* ctx, const char* fn, const mirt_pass_desc* d, bool guides, pt::FusedArgs& A, bool with_material = true) {
    if (!d || d->struct_size != sizeof(mirt_pass_desc)) return fail(ctx, MIRT_E_ARG, "%s: descriptor size mismatch", fn);
    if (!d->width || !d->height || !d->rays_per_pixel) return fail(ctx, MIRT_E_ARG, "%s: empty image", fn);
    {   // the host only ever makes k x k rays per pixel (A10 code.js:540); initTrace's k x k loops leave the tail of any other count
        // unwritten (code.cl:479-512), i.e. those rays would be whatever the buffer held -- there is nothing to reproduce
        const uint32_t k = (uint32_t)std::sqrt((double)d->rays_per_pixel);
        const uint32_t kk = (k + 1) * (k + 1) == d->rays_per_pixel ? k + 1 : k;
        if (kk * kk != d->rays_per_pixel)
            return fail(ctx, MIRT_E_ARG, "%s: rays_per_pixel %u is not a square (the lens grid is k x k, A10 code.js:540)", fn, d->rays_per_pixel);
    }
    if (int rc = check_desc_arrays(ctx, fn, d, !guides, "light/mesh")) return rc;
    if (!guides && !d->pass_index) return fail(ctx, MIRT_E_ARG, "%s: pass_index is 1-based", fn);
    const uint32_t cols = f2u_host(d->cam[14]), rows = f2u_host(d->cam[15]);
    if (cols != d->width || rows != d->height) return fail(ctx, MIRT_E_ARG, "%s: camera says %ux%u, descriptor %ux%u", fn, cols, rows, d->width, d->height);
    const uint32_t nrows = d->nrows ? d->nrows : d->height;
    if (d->row0 >= d->height || nrows > d->height - d->row0) return fail(ctx, MIRT_E_ARG, "%s: row tile [%u,+%u) outside the image", fn, d->row0, nrows);
    const uint64_t npix = (uint64_t)nrows * d->width;
    const uint64_t nrays = npix * d->rays_per_pixel;
    if (nrays > 0xFFFFFF00ull) return fail(ctx, MIRT_E_ARG, "%s: %llu rays in one tile (the kernels index a tile's rays with 32 bits); split the rows over more launches", fn, (unsigned long long)nrays);
    HIPCHK(ctx, hipSetDevice(ctx->device));

    memset(&A, 0, sizeof A);
    memcpy(A.cam, d->cam, sizeof A.cam);
    memcpy(A.bound, d->scene_bounds, sizeof A.bound);
    A.focal_length = d->focal_length; A.lens_rad = d->lens_rad;
    A.width = d->width; A.height = d->height; A.rpp = d->rays_per_pixel;
    A.row0 = d->row0; A.nrows = nrows; A.bounces = d->bounces;
    A.n_lights = guides ? 0u : d->n_lights;
    int rc;
    if ((rc = fill_sets(ctx, fn, d, A))) return rc;
    return fill_shading(ctx, d, A, with_material);
}

// The A.n_lights light records of a descriptor and, with_material, its material table: what a pass and mirt_trace_radiance shade with.  The
// caller has checked n_lights and the light array.
static int fill_shading(mirt_ctx* ctx, const mirt_pass_desc* d, pt::FusedArgs& A, bool with_material) {
    for (uint32_t l = 0; l < A.n_lights; ++l) {
        memcpy(A.lights[l].shadow, d->lights[l].shadow, 64);
        memcpy(A.lights[l].scene, d->lights[l].scene, 64);
        memcpy(A.lights[l].light, d->lights[l].light, 64);
    }
    if (!with_material) return MIRT_OK;
    int rc;
    if ((rc = need(ctx, "material", d->material, 16))) return rc;
    A.material = d->material->ptr;
    A.nmat = (uint32_t)(d->material->bytes / 16);
    return MIRT_OK;
}

// The primitive sets of a descriptor into A.sets, in upload order, validated and prepared (fill_grid): what a pass, the guides and the ray queries
// (mirt_trace_closest, mirt_trace_occluded) share.  The caller has checked n_meshes and the mesh array.
static int fill_sets(mirt_ctx* ctx, const char* fn, const mirt_pass_desc* d, pt::FusedArgs& A) {
    int rc;
    if (d->spheres && (rc = fill_grid(ctx, "spheres", d->spheres, false, true, &A.sets[A.n_sets++]))) return rc;
    if (d->triangles && (rc = fill_grid(ctx, "triangles", d->triangles, true, true, &A.sets[A.n_sets++]))) return rc;
    for (uint32_t m = 0; m < d->n_meshes; ++m)
        if ((rc = fill_grid(ctx, "mesh", &d->meshes[m], true, false, &A.sets[A.n_sets++]))) return rc;
    // one prepared copy per position buffer, laid out for ONE record count: two sets of a pass that share a buffer with different counts would have
    // the second fill_grid re-lay the copy the first set's pointers describe
    {
        const mirt_grid* gs[2 + MIRT_MAX_MESHES];
        uint32_t ng = 0;
        if (d->triangles) gs[ng++] = d->triangles;
        for (uint32_t m = 0; m < d->n_meshes; ++m) gs[ng++] = &d->meshes[m];
        for (uint32_t i = 0; i < ng; ++i)
            for (uint32_t j = i + 1; j < ng; ++j)
                if (gs[i]->prims == gs[j]->prims && gs[i]->cell_offsets->off_last != gs[j]->cell_offsets->off_last)
                    return fail(ctx, MIRT_E_ARG, "%s: two triangle sets share a position buffer but hold %u and %u slots (one prepared copy per buffer: "
                                                 "give each set its own buffer)", fn, gs[i]->cell_offsets->off_last, gs[j]->cell_offsets->off_last);
    }
    return MIRT_OK;
}

// The guide launches of an already validated tile: the optimistic / exact pair of one lane per pixel, or the exact kernel alone.
static int queue_guides(mirt_ctx* ctx, const pt::FusedArgs& A, void* nh, void* ad) {
    const uint64_t npix = (uint64_t)A.nrows * A.width;
    return queue_pair(ctx, ctx->guide_mask, A, (uint32_t)((npix + 31u) / 32u), 1u, [&](bool fast, uint32_t* mask_out, const uint32_t* mask_in) {
        pt::launch_guides(ctx->stream, A, fast, nh, ad, mask_out, mask_in);
    });
}

// mirt_render_first_pass_guided's and mirt_render_passes_guided's own buffer rules (`fn`: which), after the pass's: each guide given holds the tile's pixels x 16 B (MIRT_E_RANGE), and its bytes
// meet those of no buffer of the descriptor nor the other guide's (MIRT_E_ARG) -- the pass and the guides are written by the same launches.
// (The pass has checked the descriptor's own buffers: nothing more is asked of them here, and they count whole.)
static int guided_check_buffers(mirt_ctx* ctx, const char* fn, const mirt_pass_desc* d, mirt_buf* nh, mirt_buf* ad, uint64_t npix) {
    const CallBuf b[6] = {{"normal_hits", nh, npix * 16}, {"albedo_depth", ad, npix * 16}, {"seeds", d->seeds, 0, BUF_IN_WHOLE}, {"acu", d->acu, 0, BUF_IN_WHOLE},
                          {"pixel", d->pixel, 0, BUF_IN_WHOLE}, {"radiance", d->radiance, 0, BUF_IN_WHOLE}};
    return check_call_buffers(ctx, fn, b, d, true, "%s: a guide buffer aliases a buffer of the descriptor", "%s: normal_hits aliases albedo_depth");
}
// MIRT_GUIDED_PASS=0: mirt_render_first_pass_guided and mirt_render_passes_guided always queue the pass and then the guide launches -- an A/B and test switch, read per call
static bool guided_pass_enabled() { const char* e = getenv("MIRT_GUIDED_PASS"); return !(e && e[0] == '0'); }

static int render_pass_impl(mirt_ctx* ctx, const mirt_pass_desc* d, const PassOpts& o) {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_render_pass: unknown context");
    pt::FusedArgs A;
    int rc;
    if ((rc = pass_setup(ctx, "mirt_render_pass", d, false, A))) return rc;
    const uint32_t nrows = A.nrows;
    const uint64_t npix = (uint64_t)nrows * d->width;
    const uint64_t nrays = npix * d->rays_per_pixel;
    A.fresh = o.fresh ? 1u : 0u;
    A.passes = o.passes;
    // the frame after the last pass: 1 / (rpp * passes so far), A10 code.js:1412 -- or the recorded copyToPixel's own factor, which try_fuse_pass hands over (not a NaN)
    const float res_m = o.passes == 1u && o.tone == o.tone ? o.tone : (float)(1.0 / ((double)d->rays_per_pixel * ((double)d->pass_index + (double)(o.passes - 1u))));
    if ((rc = need(ctx, "seeds", d->seeds, nrays * 4))) return rc;
    // what is launched, worked out once (pt_pass_plan.hpp): whether the pass resolves its own pixels -- then, and only then, `acu` is optional --
    // its segments, the mask and the scratch buffer
    const pt::PassPlan plan = pt::pass_plan(pass_request(ctx, d, o));
    const bool want_out = d->pixel || d->radiance;
    ctx->last_pass_resolved = plan.resolves;
    if (!plan.null_acu_ok)
        return fail(ctx, MIRT_E_ARG, "mirt_render_pass: acu may only be null for a frame's first pass (mirt_render_first_pass) with a pixel or radiance buffer and "
                                     "rays_per_pixel dividing 256 or above 256, unless MIRT_INPASS_RESOLVE=0 (here: %s, %u rays per pixel%s)", o.fresh ? "first pass" : "NOT a first pass",
                    d->rays_per_pixel, want_out ? "" : ", no output buffer");
    if (d->acu && (rc = need(ctx, "acu", d->acu, nrays * kAcuBytes))) return rc;
    A.seeds = (int32_t*)d->seeds->ptr;
    A.acu = d->acu ? d->acu->ptr : nullptr;
    const uint64_t frames = o.every ? o.passes : (uint64_t)o.frame + 1u;   // frames the pixel / radiance buffers hold, back to back
    if (d->pixel && (rc = need(ctx, "pixel", d->pixel, npix * 4 * frames))) return rc;
    if (d->radiance && (rc = need(ctx, "radiance", d->radiance, npix * 16 * frames))) return rc;
    void* const pixel_ptr = d->pixel ? (char*)d->pixel->ptr + (size_t)o.frame * npix * 4 : nullptr;
    void* const radiance_ptr = d->radiance ? (char*)d->radiance->ptr + (size_t)o.frame * npix * 16 : nullptr;
    if (o.every && !plan.resolves) return fail(ctx, MIRT_E_ARG, "mirt_render_passes: a frame after every pass in one launch needs a pass that resolves in the kernel");
    // the column streams live in seeds[0..width): only the tile that owns row 0 holds them
    if (A.rpp == 1 && d->row0 != 0) return fail(ctx, MIRT_E_ARG, "mirt_render_pass: rays_per_pixel == 1 couples rows through seeds[col] (A10 code.cl:429); render it as one tile");
    // the guides beside the pass (mirt_render_first_pass_guided): the last of the checks -- nothing has been queued yet -- and the route
    const bool guided = o.guide_nh || o.guide_ad;
    if (guided && (rc = guided_check_buffers(ctx, o.guide_fn, d, o.guide_nh, o.guide_ad, npix))) return rc;
    void* const guide_nh = o.guide_nh ? o.guide_nh->ptr : nullptr;
    void* const guide_ad = o.guide_ad ? o.guide_ad->ptr : nullptr;
    const auto rule = [&] {   // (asked only of a guided call: the pairing is read from the environment)
        return o.guide_mode == PassOpts::GUIDES_FIRST_PASS ? pt::fused_guides_in_pass(plan, o.passes)
             : o.guide_mode == PassOpts::GUIDES_PASSES     ? pt::fused_guides_in_passes(plan, o.passes, pt::fused_multipass_default(A), pt::fused_has_grids(A))
                                                           : false;
    };
    const bool guides_in_pass = guided && guided_pass_enabled() && rule();
    if (guides_in_pass) { A.guide_nh = guide_nh; A.guide_ad = guide_ad; }
    if (plan.scratch_bytes && (rc = ensure_scratch(ctx, (size_t)plan.scratch_bytes))) return rc;
    char* const scratch = (char*)ctx->scratch;
    if (plan.resolves) {
        A.resolve = 1u;
        // a pixel of more than 256 rays: its sums travel from launch to launch through memory (FusedArgs::seg_off)
        A.radiance = plan.sums.bytes ? scratch + plan.sums.off : radiance_ptr;
        A.res_m = res_m;
        if (o.every) {
            A.every = 1u;
            A.pass_index = d->pass_index;
        }
    }
    // every frame, more than 256 rays per pixel: the two arrays the segments' sums alternate between (FusedArgs::carry, pt_pass_plan.hpp pass_segment)
    void* const carry[2] = {plan.carry[0].bytes ? scratch + plan.carry[0].off : radiance_ptr, scratch + plan.carry[1].off};
    if (plan.lens.bytes) {
        A.uv = scratch + plan.lens.off;
        pt::launch_lensDraws(ctx->stream, A.seeds, scratch + plan.lens.off, d->width, d->height, d->width, d->height, d->row0, nrows);
    }
    if (ctx->profiling && !ctx->capturing && o.mark_start) HIPCHK(ctx, hipEventRecord(ctx->pe[0], ctx->stream));
    const bool pair = optimistic(ctx, A);
    DeferMask& m = ctx->pass_mask;
    if (pair) {
        // optimistic kernel (exact cheap divisions inside their window) + exact kernel over the samples that left the window:
        // the second launch walks the first one's bit mask on the device, so the pair is queued without a host round trip
        // one bit per sample -- or, resolving in the pass, per block of 256 samples (pt_kernels_fused.hip)
        if (m.bytes < DeferMask::bytes_for(plan.mask_words)) {   // a recording holds the mask's address: it cannot grow inside one, and a graph recorded before is stale
            NOT_WHILE_CAPTURING(ctx, "growing the deferred-sample mask");
            ctx->defer_gen++;
        }
        if (ctx->capturing) ctx->cap_defer = true;
        if ((rc = grow_and_clear(ctx, m, plan.mask_words))) return rc;
    }
    // One launch -- optimistic: one pair of launches -- per segment of the plan, in ray order, each on its own region of the mask; the redo launch of
    // a segment runs before the next segment's launches read the sums it leaves (stream order).  A pass that does not resolve is one segment.
    for (uint32_t i = 0; i < plan.n_segments; ++i) {
        const pt::PassSegment seg = pt::pass_segment(plan, i);
        A.seg_off = seg.off;
        A.seg_len = seg.len;
        A.seg_pitch = seg.pitch;
        A.pixel = seg.writes_pixel ? pixel_ptr : nullptr;
        if (plan.carries) {
            A.radiance = carry[seg.carry_write];
            A.carry = carry[seg.carry_read];
        }
        if (pair) {
            pt::launch_fused(ctx->stream, A, true, m.bits() + seg.mask_first, nullptr, 0);
            pt::launch_fused(ctx->stream, A, false, nullptr, m.bits() + seg.mask_first, seg.mask_words);
        } else {
            pt::launch_fused(ctx->stream, A, false, nullptr, nullptr, 0);
        }
    }
    m.words = pair ? plan.mask_words : 0u;
    if (pair) m.unit = plan.mask_unit;
    if (ctx->profiling && !ctx->capturing) HIPCHK(ctx, hipEventRecord(ctx->pe[1], ctx->stream));
    if (!plan.resolves && want_out) pt::launch_copyToPixel(ctx->stream, pixel_ptr, A.acu, res_m, (uint32_t)npix, A.rpp, (uint32_t)npix, radiance_ptr);
    if (ctx->profiling && !ctx->capturing) { HIPCHK(ctx, hipEventRecord(ctx->pe[2], ctx->stream)); ctx->pe_valid = true; }
    if (guides_in_pass) ctx->guided_passes++;
    else if (guided && o.guide_mode != PassOpts::GUIDES_CHECK_ONLY && (rc = queue_guides(ctx, A, guide_nh, guide_ad))) return rc;   // everywhere else: exactly what mirt_render_guides queues
    HIPCHK(ctx, hipGetLastError());
    d->seeds->version++;
    if (d->acu) d->acu->version++;
    if (o.guide_nh && o.guide_mode != PassOpts::GUIDES_CHECK_ONLY) o.guide_nh->version++;
    if (o.guide_ad && o.guide_mode != PassOpts::GUIDES_CHECK_ONLY) o.guide_ad->version++;
    return MIRT_OK;
}

int mirt_render_pass(mirt_ctx* ctx, const mirt_pass_desc* d) try { if (live_has(ctx)) FLUSH_PENDING(ctx); return render_pass_impl(ctx, d, PassOpts{}); } MIRT_CATCH("mirt_render_pass", return MIRT_E_DEVICE)
int mirt_render_first_pass(mirt_ctx* ctx, const mirt_pass_desc* d) try {
    if (live_has(ctx)) FLUSH_PENDING(ctx);
    PassOpts o;
    o.fresh = true;
    return render_pass_impl(ctx, d, o);
} MIRT_CATCH("mirt_render_first_pass", return MIRT_E_DEVICE)
// mirt_render_first_pass + mirt_render_guides in one call: the checks of both before anything is queued, then -- where the plan allows
// (pt_pass_plan.hpp fused_guides_in_pass) -- the pass's own launches write the guides (k_fusedPass GUIDES), elsewhere the guide launches follow.
int mirt_render_first_pass_guided(mirt_ctx* ctx, const mirt_pass_desc* d, mirt_buf* normal_hits, mirt_buf* albedo_depth) try {
    ENTRY_PROLOGUE(ctx, "mirt_render_first_pass_guided");
    if (!normal_hits && !albedo_depth) return fail(ctx, MIRT_E_ARG, "mirt_render_first_pass_guided: normal_hits and albedo_depth are both NULL (either may be, not both)");
    if (d && d->struct_size == sizeof(mirt_pass_desc) && d->rays_per_pixel == 1u)
        return fail(ctx, MIRT_E_ARG, "mirt_render_first_pass_guided: rays_per_pixel == 1 draws its lens sample from seeds[col] (A10 code.cl:429); the guides are defined "
                                     "for the un-jittered k x k lens grid, rays_per_pixel >= 4 (mirt_render_guides)");
    PassOpts o;
    o.fresh = true;
    o.guide_nh = normal_hits;
    o.guide_ad = albedo_depth;
    return render_pass_impl(ctx, d, o);
} MIRT_CATCH("mirt_render_first_pass_guided", return MIRT_E_DEVICE)

// n_passes progressive passes in one call: the same results as mirt_render_first_pass (MIRT_PASSES_FRESH) or mirt_render_pass at pass_index,
// then mirt_render_pass at pass_index + 1 .. pass_index + n_passes - 1 -- one launch (per block of a pixel's rays) that runs every sample through
// all of them (pt_kernels_fused.hip k_fusedPass MULTI).
// (the body of mirt_render_passes and of mirt_render_passes_guided, which gives one guide buffer at least)
static int render_passes_impl(mirt_ctx* ctx, const mirt_pass_desc* d, uint32_t n_passes, uint32_t flags, mirt_buf* guide_nh, mirt_buf* guide_ad) {
    const bool guided = guide_nh || guide_ad;
    if (!d || d->struct_size != sizeof(mirt_pass_desc)) return fail(ctx, MIRT_E_ARG, "mirt_render_passes: descriptor size mismatch");
    if (flags & ~(MIRT_PASSES_FRESH | MIRT_PASSES_EVERY_FRAME)) return fail(ctx, MIRT_E_ARG, "mirt_render_passes: unknown flags 0x%x", flags);
    if (n_passes < 1u || n_passes > MIRT_MAX_PASSES_PER_CALL)
        return fail(ctx, MIRT_E_ARG, "mirt_render_passes: n_passes %u outside 1..%u (one launch lasts about n_passes single passes)", n_passes, MIRT_MAX_PASSES_PER_CALL);
    if (d->pass_index > UINT32_MAX - (n_passes - 1u)) return fail(ctx, MIRT_E_ARG, "mirt_render_passes: pass_index %u + %u passes overflows", d->pass_index, n_passes);
    PassOpts o;
    o.fresh = (flags & MIRT_PASSES_FRESH) != 0u;
    o.passes = n_passes;
    o.every = (flags & MIRT_PASSES_EVERY_FRAME) != 0u;
    const pt::PassPlan plan = pt::pass_plan(pass_request(ctx, d, o));   // (of the call as asked for: its null-acu verdict and its route)
    if (!plan.null_acu_ok_passes)
        return fail(ctx, MIRT_E_ARG, "mirt_render_passes: acu may only be NULL with MIRT_PASSES_FRESH, a pixel or radiance buffer and rays_per_pixel > 1 dividing 256 "
                                     "or above 256, unless MIRT_INPASS_RESOLVE=0 (here: %s, %u rays per pixel%s)", o.fresh ? "fresh" : "NOT fresh",
                    d->rays_per_pixel, d->pixel || d->radiance ? "" : ", no output buffer");
    // MIRT_PASSES_EVERY_FRAME: pixel / radiance hold n_passes frames; both are checked before anything runs
    if (o.every) {
        if (!d->pixel && !d->radiance) return fail(ctx, MIRT_E_ARG, "mirt_render_passes: MIRT_PASSES_EVERY_FRAME needs a pixel or radiance buffer for the frames");
        const uint64_t npix = plan.npix;
        if (d->pixel && live_has(d->pixel) && (uint64_t)d->pixel->bytes < npix * 4 * n_passes)
            return fail(ctx, MIRT_E_ARG, "mirt_render_passes: pixel holds %zu bytes, %u frames of %llu pixels need %llu", d->pixel->bytes, n_passes,
                        (unsigned long long)npix, (unsigned long long)(npix * 4 * n_passes));
        if (d->radiance && live_has(d->radiance) && (uint64_t)d->radiance->bytes < npix * 16 * n_passes)
            return fail(ctx, MIRT_E_ARG, "mirt_render_passes: radiance holds %zu bytes, %u frames of %llu pixels need %llu", d->radiance->bytes, n_passes,
                        (unsigned long long)npix, (unsigned long long)(npix * 16 * n_passes));
    }
    if (guided) {
        o.guide_nh = guide_nh;
        o.guide_ad = guide_ad;
        o.guide_fn = "mirt_render_passes_guided";
        o.guide_mode = PassOpts::GUIDES_PASSES;
    }
    // one launch: the frame after the last pass, or -- where the passes resolve in the kernel -- every pass's frame
    if (plan.route != pt::ROUTE_ORDINARY_PASSES) return render_pass_impl(ctx, d, o);
    // elsewhere ordinary passes, each writing its own frame slot when every frame is asked for
    mirt_pass_desc p = *d;
    for (uint32_t i = 0; i < n_passes; ++i) {
        p.pass_index = d->pass_index + i;
        PassOpts one;
        one.fresh = o.fresh && i == 0u;
        one.mark_start = i == 0u;
        one.frame = o.every ? i : 0u;
        if (guided && (i == 0u || i + 1u == n_passes)) {   // the guides' checks before the first pass queues anything, their launches behind the last
            one.guide_nh = guide_nh;
            one.guide_ad = guide_ad;
            one.guide_fn = o.guide_fn;
            one.guide_mode = i + 1u == n_passes ? PassOpts::GUIDES_BEHIND : PassOpts::GUIDES_CHECK_ONLY;
        }
        const int rc = render_pass_impl(ctx, &p, one);
        if (rc) return rc;
    }
    return MIRT_OK;
}
int mirt_render_passes(mirt_ctx* ctx, const mirt_pass_desc* d, uint32_t n_passes, uint32_t flags) try {
    ENTRY_PROLOGUE(ctx, "mirt_render_passes");
    return render_passes_impl(ctx, d, n_passes, flags, nullptr, nullptr);
} MIRT_CATCH("mirt_render_passes", return MIRT_E_DEVICE)
// mirt_render_passes + mirt_render_guides in one call: the checks of both before anything is queued, then -- where the plan allows
// (pt_pass_plan.hpp fused_guides_in_passes) -- the multi-pass launch writes the guides in its first pass (k_fusedPass GUIDES with MULTI), elsewhere
// the guide launches follow what mirt_render_passes queues.
int mirt_render_passes_guided(mirt_ctx* ctx, const mirt_pass_desc* d, uint32_t n_passes, uint32_t flags, mirt_buf* normal_hits, mirt_buf* albedo_depth) try {
    ENTRY_PROLOGUE(ctx, "mirt_render_passes_guided");
    if (!normal_hits && !albedo_depth) return fail(ctx, MIRT_E_ARG, "mirt_render_passes_guided: normal_hits and albedo_depth are both NULL (either may be, not both)");
    if (d && d->struct_size == sizeof(mirt_pass_desc) && d->rays_per_pixel == 1u)
        return fail(ctx, MIRT_E_ARG, "mirt_render_passes_guided: rays_per_pixel == 1 draws its lens sample from seeds[col] (A10 code.cl:429); the guides are defined "
                                     "for the un-jittered k x k lens grid, rays_per_pixel >= 4 (mirt_render_guides)");
    return render_passes_impl(ctx, d, n_passes, flags, normal_hits, albedo_depth);
} MIRT_CATCH("mirt_render_passes_guided", return MIRT_E_DEVICE)

// First-hit guide buffers of the tile (pt_kernels_guides.hip): the descriptor's geometry through the checks of mirt_render_pass, then one launch
// -- or the optimistic / exact pair -- of one lane per pixel.  Nothing but the two outputs is written.
int mirt_render_guides(mirt_ctx* ctx, const mirt_pass_desc* d, mirt_buf* normal_hits, mirt_buf* albedo_depth) try {
    ENTRY_PROLOGUE(ctx, "mirt_render_guides");
    if (!normal_hits && !albedo_depth) return fail(ctx, MIRT_E_ARG, "mirt_render_guides: normal_hits and albedo_depth are both NULL (either may be, not both)");
    if (d && d->struct_size == sizeof(mirt_pass_desc) && d->rays_per_pixel == 1u)
        return fail(ctx, MIRT_E_ARG, "mirt_render_guides: rays_per_pixel == 1 draws its lens sample from seeds[col] (A10 code.cl:429), so its guides would change "
                                     "with the seeds and from pass to pass; the guides are defined for the un-jittered k x k lens grid, rays_per_pixel >= 4");
    pt::FusedArgs A;
    int rc;
    if ((rc = pass_setup(ctx, "mirt_render_guides", d, true, A))) return rc;
    const uint64_t npix = (uint64_t)A.nrows * A.width;
    const CallBuf io[2] = {{"normal_hits", normal_hits, npix * 16}, {"albedo_depth", albedo_depth, npix * 16}};
    if ((rc = check_call_buffers(ctx, nullptr, io, d, false, nullptr, nullptr))) return rc;   // (bare labels, and no aliasing rule: the call never had one)
    if ((rc = queue_guides(ctx, A, normal_hits ? normal_hits->ptr : nullptr, albedo_depth ? albedo_depth->ptr : nullptr))) return rc;
    return finish_call(ctx, io, 2);
} MIRT_CATCH("mirt_render_guides", return MIRT_E_DEVICE)

// Ambient occlusion of the first hit (pt_kernels_rays.hip k_ao): the guides' checks without the material, the call's own, then one launch -- or the
// optimistic / exact pair, per pixel -- of one lane per pixel.  Every check comes before anything is queued; nothing but ao_out is written.
int mirt_render_ao(mirt_ctx* ctx, const mirt_pass_desc* d, const mirt_ao_desc* ao, mirt_buf* ao_out) try {
    ENTRY_PROLOGUE(ctx, "mirt_render_ao");
    if (!ao || ao->struct_size != sizeof(mirt_ao_desc)) return fail(ctx, MIRT_E_ARG, "mirt_render_ao: AO descriptor size mismatch");
    if (!ao->samples || ao->samples > MIRT_AO_MAX_SAMPLES) return fail(ctx, MIRT_E_ARG, "mirt_render_ao: samples %u outside 1..%u", ao->samples, MIRT_AO_MAX_SAMPLES);
    if (!(ao->radius > 0.0f)) return fail(ctx, MIRT_E_ARG, "mirt_render_ao: radius %g is not above 0", (double)ao->radius);
    if (!(ao->bias >= 0.0f) || std::isinf(ao->bias)) return fail(ctx, MIRT_E_ARG, "mirt_render_ao: bias %g is not a finite number >= 0", (double)ao->bias);
    if (!ao_out) return fail(ctx, MIRT_E_ARG, "mirt_render_ao: ao_out is NULL");
    if (d && d->struct_size == sizeof(mirt_pass_desc)) {
        if (d->rays_per_pixel == 1u)
            return fail(ctx, MIRT_E_ARG, "mirt_render_ao: rays_per_pixel == 1 draws its lens sample from seeds[col] (A10 code.cl:429); the first hit is defined "
                                         "for the un-jittered k x k lens grid, rays_per_pixel >= 4 (mirt_render_guides)");
        if (!d->seeds) return fail(ctx, MIRT_E_ARG, "mirt_render_ao: seeds is NULL (the AO rays draw from them; they are not written)");
    }
    pt::FusedArgs A;
    int rc;
    if ((rc = pass_setup(ctx, "mirt_render_ao", d, true, A, false))) return rc;
    const uint64_t npix = (uint64_t)A.nrows * A.width;
    const uint64_t nrays = npix * A.rpp;
    // the output is read by nobody and no input is written: the bytes the call writes, against the seeds' and the geometry's buffers whole
    const CallBuf io[2] = {{"seeds", d->seeds, nrays * 4, BUF_IN_WHOLE}, {"ao_out", ao_out, npix * 8}};
    if ((rc = check_call_buffers(ctx, "mirt_render_ao", io, d, false, "%s: ao_out's bytes meet the seeds' or a geometry buffer's", nullptr))) return rc;
    A.seeds = (int32_t*)d->seeds->ptr;
    rc = queue_pair(ctx, ctx->ao_mask, A, (uint32_t)((npix + 31u) / 32u), 1u, [&](bool fast, uint32_t* mask_out, const uint32_t* mask_in) {
        pt::launch_ao(ctx->stream, A, fast, ao->samples, ao->radius, ao->bias, ao_out->ptr, mask_out, mask_in);
    });
    return rc ? rc : finish_call(ctx, io, 2);
} MIRT_CATCH("mirt_render_ao", return MIRT_E_DEVICE)

int mirt_ao_deferred(mirt_ctx* ctx, uint64_t* pixels) try {
    ENTRY_PROLOGUE(ctx, "mirt_ao_deferred");
    return count_deferred(ctx, "mirt_ao_deferred", ctx->ao_mask, pixels);
} MIRT_CATCH("mirt_ao_deferred", return MIRT_E_DEVICE)

// ---- ray queries (pt_kernels_rays.hip): mirt_trace_closest and mirt_trace_occluded.  Every check comes before anything is queued; then one launch
// -- or the optimistic / exact pair, per ray -- of one lane per ray.  Nothing but the outputs is written.
static int trace_impl(mirt_ctx* ctx, const char* fn, const mirt_pass_desc* d, mirt_buf* rays, uint64_t count, mirt_buf* hits, mirt_buf* sets, mirt_buf* occluded, bool any) {
    ENTRY_PROLOGUE(ctx, fn);
    if (!d || d->struct_size != sizeof(mirt_pass_desc)) return fail(ctx, MIRT_E_ARG, "%s: descriptor size mismatch", fn);
    if (count > 0xFFFFFF00ull) return fail(ctx, MIRT_E_ARG, "%s: %llu rays in one call (the kernels index a call's rays with 32 bits); split the batch", fn, (unsigned long long)count);
    if (!any && !hits && !sets) return fail(ctx, MIRT_E_ARG, "%s: hits and sets are both NULL (either may be, not both)", fn);
    if (any && !occluded) return fail(ctx, MIRT_E_ARG, "%s: occluded is NULL", fn);
    int rc;
    if ((rc = check_desc_arrays(ctx, fn, d, false, "mesh"))) return rc;
    if (!rays) return fail(ctx, MIRT_E_HANDLE, "%s: rays is NULL", fn);
    // an output is read by nobody and no input is written: the bytes the call touches, and the geometry's buffers whole
    const CallBuf io[4] = {{"rays", rays, count * 32, BUF_IN}, {"hits", hits, count * 32}, {"sets", sets, count * 4}, {"occluded", occluded, count}};
    if ((rc = check_call_buffers(ctx, fn, io, d, false, "%s: an output's bytes meet the rays' or a geometry buffer's", "%s: hits aliases sets"))) return rc;
    if (!count) return MIRT_OK;   // (nothing is queued, and the counter of the last batch stays)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pt::FusedArgs A;
    memset(&A, 0, sizeof A);
    if ((rc = fill_sets(ctx, fn, d, A))) return rc;
    void* const hp = hits ? hits->ptr : nullptr;
    uint32_t* const sp = sets ? (uint32_t*)sets->ptr : nullptr;
    uint8_t* const op = occluded ? (uint8_t*)occluded->ptr : nullptr;
    rc = queue_pair(ctx, ctx->ray_mask, A, (uint32_t)((count + 31u) / 32u), 1u, [&](bool fast, uint32_t* mask_out, const uint32_t* mask_in) {
        pt::launch_rays(ctx->stream, A, fast, rays->ptr, (uint32_t)count, hp, sp, op, mask_out, mask_in);
    });
    return rc ? rc : finish_call(ctx, io, 4);
}

int mirt_trace_closest(mirt_ctx* ctx, const mirt_pass_desc* d, mirt_buf* rays, uint64_t count, mirt_buf* hits, mirt_buf* sets) try {
    return trace_impl(ctx, "mirt_trace_closest", d, rays, count, hits, sets, nullptr, false);
} MIRT_CATCH("mirt_trace_closest", return MIRT_E_DEVICE)

int mirt_trace_occluded(mirt_ctx* ctx, const mirt_pass_desc* d, mirt_buf* rays, uint64_t count, mirt_buf* occluded) try {
    return trace_impl(ctx, "mirt_trace_occluded", d, rays, count, nullptr, nullptr, occluded, true);
} MIRT_CATCH("mirt_trace_occluded", return MIRT_E_DEVICE)

int mirt_trace_deferred(mirt_ctx* ctx, uint64_t* rays) try {
    ENTRY_PROLOGUE(ctx, "mirt_trace_deferred");
    return count_deferred(ctx, "mirt_trace_deferred", ctx->ray_mask, rays);
} MIRT_CATCH("mirt_trace_deferred", return MIRT_E_DEVICE)

// ---- path radiance of caller-supplied rays (pt_kernels_rays.hip k_traceRadiance): mirt_trace_radiance.  Every check comes before anything is
// queued; then one launch -- or the optimistic / exact pair, per ray -- of one lane per ray.  Nothing but seeds and radiance is written.
int mirt_trace_radiance(mirt_ctx* ctx, const mirt_pass_desc* d, const mirt_radiance_desc* rd, mirt_buf* rays, uint64_t count, mirt_buf* seeds, mirt_buf* radiance) try {
    const char* const fn = "mirt_trace_radiance";
    ENTRY_PROLOGUE(ctx, fn);
    if (!d || d->struct_size != sizeof(mirt_pass_desc)) return fail(ctx, MIRT_E_ARG, "%s: descriptor size mismatch", fn);
    if (!rd || rd->struct_size != sizeof(mirt_radiance_desc)) return fail(ctx, MIRT_E_ARG, "%s: radiance descriptor size mismatch", fn);
    if (!rd->samples || rd->samples > MIRT_RADIANCE_MAX_SAMPLES) return fail(ctx, MIRT_E_ARG, "%s: samples %u outside 1..%u", fn, rd->samples, MIRT_RADIANCE_MAX_SAMPLES);
    if (rd->flags & ~(MIRT_RADIANCE_ACCUMULATE | MIRT_RADIANCE_NO_EMITTERS)) return fail(ctx, MIRT_E_ARG, "%s: unknown flags 0x%x", fn, rd->flags);
    if (rd->reserved) return fail(ctx, MIRT_E_ARG, "%s: reserved is %u, not 0", fn, rd->reserved);
    if (count > 0xFFFFFF00ull) return fail(ctx, MIRT_E_ARG, "%s: %llu rays in one call (the kernels index a call's rays with 32 bits); split the batch", fn, (unsigned long long)count);
    if (!seeds || !radiance) return fail(ctx, MIRT_E_ARG, "%s: %s is NULL", fn, seeds ? "radiance" : "seeds");
    int rc;
    if ((rc = check_desc_arrays(ctx, fn, d, true, "light/mesh"))) return rc;
    if (!rays) return fail(ctx, MIRT_E_HANDLE, "%s: rays is NULL", fn);
    // seeds and radiance are both written: the bytes the call touches of them, against the rays', the geometry's buffers and the material whole
    const CallBuf io[3] = {{"rays", rays, count * 32, BUF_IN}, {"seeds", seeds, count * 4}, {"radiance", radiance, count * 16}};
    if ((rc = check_call_buffers(ctx, fn, io, d, true, "%s: the seeds' or the radiance's bytes meet the rays', a geometry buffer's or the material's", "%s: seeds aliases radiance"))) return rc;
    if (!count) return MIRT_OK;   // (nothing is queued, and the counter of the last batch stays)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pt::FusedArgs A;
    memset(&A, 0, sizeof A);
    A.bounces = d->bounces;
    A.n_lights = d->n_lights;
    if ((rc = fill_sets(ctx, fn, d, A))) return rc;
    if ((rc = fill_shading(ctx, d, A, true))) return rc;
    rc = queue_pair(ctx, ctx->rad_mask, A, (uint32_t)((count + 31u) / 32u), 1u, [&](bool fast, uint32_t* mask_out, const uint32_t* mask_in) {
        pt::launch_radiance(ctx->stream, A, fast, rays->ptr, (uint32_t)count, rd->samples, rd->flags, (int32_t*)seeds->ptr, radiance->ptr, mask_out, mask_in);
    });
    return rc ? rc : finish_call(ctx, io, 3);
} MIRT_CATCH("mirt_trace_radiance", return MIRT_E_DEVICE)

int mirt_radiance_deferred(mirt_ctx* ctx, uint64_t* rays) try {
    ENTRY_PROLOGUE(ctx, "mirt_radiance_deferred");
    return count_deferred(ctx, "mirt_radiance_deferred", ctx->rad_mask, rays);
} MIRT_CATCH("mirt_radiance_deferred", return MIRT_E_DEVICE)

// ---- panoramic, fisheye and orthographic cameras (pt_kernels_rays.hip k_viewRays, k_viewPass): mirt_view_rays, mirt_render_view.  The rules of
// the descriptor and the launch plan are pt_view_plan.hpp's (host-only, CPU-tested); here are their messages.  Every check comes before anything
// is queued.
static_assert(sizeof(pt::ViewDesc) == sizeof(mirt_view_desc) && offsetof(pt::ViewDesc, eye) == offsetof(mirt_view_desc, eye) &&
              offsetof(pt::ViewDesc, half_w) == offsetof(mirt_view_desc, half_w) && offsetof(pt::ViewDesc, tone) == offsetof(mirt_view_desc, tone),
              "pt_view_plan.hpp restates the header's descriptor");
static_assert(pt::kViewOrthographic == MIRT_VIEW_ORTHOGRAPHIC && pt::kViewEquirect == MIRT_VIEW_EQUIRECT && pt::kViewFisheye == MIRT_VIEW_FISHEYE &&
              pt::kViewAccumulate == MIRT_VIEW_ACCUMULATE && pt::kViewStatusArg == MIRT_E_ARG, "pt_view_plan.hpp restates the header's constants");
static int view_verdict(mirt_ctx* ctx, const char* fn, pt::ViewVerdict v, const pt::ViewDesc& d) {
    const int code = pt::view_status(v);
    switch (v) {
        case pt::VIEW_OK: return MIRT_OK;
        case pt::VIEW_STRUCT_SIZE: return fail(ctx, code, "%s: view descriptor size mismatch", fn);
        case pt::VIEW_MODEL: return fail(ctx, code, "%s: unknown model %u", fn, d.model);
        case pt::VIEW_FLAGS: return fail(ctx, code, "%s: unknown flags 0x%x", fn, d.flags);
        case pt::VIEW_SAMPLES: return fail(ctx, code, "%s: k = %u is not 1, 2, 4, 8 or 16", fn, d.k);
        case pt::VIEW_EXTENT: return fail(ctx, code, "%s: image %u x %u outside 1..65535", fn, d.width, d.height);
        case pt::VIEW_TILE: return fail(ctx, code, "%s: row tile [%u,+%u) outside the image", fn, d.row0, pt::view_tile_rows(d));
        case pt::VIEW_TILE_RAYS: return fail(ctx, code, "%s: a tile of more than 2^32 - 256 rays (the kernels index a tile's rays with 32 bits); render fewer rows per call", fn);
        case pt::VIEW_BASIS: return fail(ctx, code, "%s: a component of eye, right, up or forward is not finite", fn);
        case pt::VIEW_ORTHO_WINDOW: return fail(ctx, code, "%s: ORTHOGRAPHIC half extents %g x %g are not finite numbers above 0", fn, (double)d.half_w, (double)d.half_h);
        case pt::VIEW_FISHEYE_ANGLE: return fail(ctx, code, "%s: FISHEYE half_angle %g is not in (0, pi]", fn, (double)d.half_angle);
        case pt::VIEW_T_MIN: return fail(ctx, code, "%s: t_min %g is not a finite number >= 0", fn, (double)d.t_min);
        case pt::VIEW_T_MAX: return fail(ctx, code, "%s: t_max %g is not above t_min %g", fn, (double)d.t_max, (double)d.t_min);
        case pt::VIEW_TONE: return fail(ctx, code, "%s: tone %g is not a finite number above 0 (it is read because a pixel buffer is given)", fn, (double)d.tone);
        case pt::VIEW_NO_SEEDS: return fail(ctx, code, "%s: seeds is NULL", fn);
        case pt::VIEW_NO_OUTPUT: return fail(ctx, code, "%s: radiance and pixel are both NULL (either may be, not both)", fn);
        case pt::VIEW_ACCUMULATE_NEEDS_RADIANCE: return fail(ctx, code, "%s: MIRT_VIEW_ACCUMULATE without a radiance buffer to go on from", fn);
        case pt::VIEW_NO_GUIDE: return fail(ctx, code, "%s: normal_hits and albedo_depth are both NULL (either may be, not both)", fn);
        case pt::VIEW_AO_STRUCT_SIZE: return fail(ctx, code, "%s: AO descriptor size mismatch", fn);
        case pt::VIEW_AO_SAMPLES: return fail(ctx, code, "%s: samples outside 1..%u", fn, MIRT_AO_MAX_SAMPLES);
        case pt::VIEW_AO_RADIUS: return fail(ctx, code, "%s: radius is not above 0", fn);
        case pt::VIEW_AO_BIAS: return fail(ctx, code, "%s: bias is not a finite number >= 0", fn);
        case pt::VIEW_AO_NO_SEEDS: return fail(ctx, code, "%s: seeds is NULL (the AO rays draw from them; they are not written)", fn);
        case pt::VIEW_AO_NO_OUTPUT: return fail(ctx, code, "%s: ao_out is NULL", fn);
        case pt::VIEW_BATCH_TILE: case pt::VIEW_BATCH_NO_CAMERAS: case pt::VIEW_BATCH_CAMERA: case pt::VIEW_BATCH_RAYS: break;   // view_batch_verdict's, below
    }
    return fail(ctx, MIRT_E_ARG, "%s: view descriptor refused", fn);
}
static pt::ViewArgs view_args(const pt::ViewDesc& d, const pt::ViewPlan& plan) {
    pt::ViewArgs V;
    memset(&V, 0, sizeof V);
    V.model = d.model; V.width = d.width; V.height = d.height; V.k = d.k; V.row0 = d.row0; V.nrows = plan.nrows;
    for (int c = 0; c < 3; ++c) { V.eye[c] = d.eye[c]; V.right[c] = d.right[c]; V.up[c] = d.up[c]; V.forward[c] = d.forward[c]; }
    V.half_w = d.half_w; V.half_h = d.half_h; V.half_angle = d.half_angle; V.t_min = d.t_min; V.t_max = d.t_max;
    return V;
}

int mirt_view_rays(mirt_ctx* ctx, const mirt_view_desc* vd, mirt_buf* rays) try {
    const char* const fn = "mirt_view_rays";
    ENTRY_PROLOGUE(ctx, fn);
    if (!vd || vd->struct_size != sizeof(mirt_view_desc)) return fail(ctx, MIRT_E_ARG, "%s: view descriptor size mismatch", fn);
    pt::ViewDesc d;
    memcpy(&d, vd, sizeof d);
    int rc;
    if ((rc = view_verdict(ctx, fn, pt::view_check_desc(d), d))) return rc;
    const pt::ViewPlan plan = pt::view_plan(d);
    if (!rays) return fail(ctx, MIRT_E_HANDLE, "%s: rays is NULL", fn);
    if ((rc = need(ctx, "mirt_view_rays rays", rays, plan.rays * 32))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pt::launch_viewRays(ctx->stream, view_args(d, plan), rays->ptr);
    HIPCHK(ctx, hipGetLastError());
    rays->version++;
    return MIRT_OK;
} MIRT_CATCH("mirt_view_rays", return MIRT_E_DEVICE)

// The guide launches of an already validated tile of a view camera: the optimistic / exact pair of one lane per pixel, or the exact kernel alone
// (the mask is mirt_render_guides's allocation: both are a bit per pixel, cleared by the call that uses them).
static int queue_view_guides(mirt_ctx* ctx, const pt::FusedArgs& A, const pt::ViewArgs& V, const pt::ViewPlan& plan, void* nh, void* ad) {
    const pt::ViewGuidesPlan g = pt::view_guides_plan(plan);
    return queue_pair(ctx, ctx->guide_mask, A, g.mask_words, 1u, [&](bool fast, uint32_t* mask_out, const uint32_t* mask_in) {
        pt::launch_viewGuides(ctx->stream, A, V, g.blocks, fast, nh, ad, mask_out, mask_in);
    });
}
// ... and of a batch's stacked image (k_viewGuidesBatch): the same pair and mask, one lane and one bit per pixel of all the frames
static int queue_view_guides_batch(mirt_ctx* ctx, const pt::FusedArgs& A, const pt::ViewBatchArgs& VB, const pt::ViewBatchPlan& bplan, void* nh, void* ad) {
    const pt::ViewGuidesPlan g = pt::view_batch_pixel_plan(bplan);
    return queue_pair(ctx, ctx->guide_mask, A, g.mask_words, 1u, [&](bool fast, uint32_t* mask_out, const uint32_t* mask_in) {
        pt::launch_viewGuidesBatch(ctx->stream, A, VB, g.blocks, fast, nh, ad, mask_out, mask_in);
    });
}
// MIRT_GUIDED_VIEW=0: mirt_render_view_guided (and its batch) always queues the frame and then the guide launches -- an A/B and test switch, read per call
static bool guided_view_enabled() { const char* e = getenv("MIRT_GUIDED_VIEW"); return !(e && e[0] == '0'); }

// ---- batched view cameras (mirt_view_rays_batch, mirt_render_view_batch, mirt_view_guides_batch, mirt_render_view_guided_batch,
// mirt_view_ao_batch): n_frames cameras' frames of one descriptor as ONE image of n_frames * height rows through k_viewRaysBatch,
// k_viewPassBatch, k_viewGuidesBatch and k_viewAoBatch (pt_kernels_view_batch.hip).  The checks and the plan are pt_view_plan.hpp's
// (view_check_batch, view_batch_plan); here are the messages and the camera table.
static_assert(sizeof(pt::ViewCamera) == sizeof(mirt_view_camera) && sizeof(mirt_view_camera) == 48 && offsetof(pt::ViewCamera, right) == offsetof(mirt_view_camera, right) &&
              offsetof(pt::ViewCamera, up) == offsetof(mirt_view_camera, up) && offsetof(pt::ViewCamera, forward) == offsetof(mirt_view_camera, forward),
              "pt_view_plan.hpp restates the header's camera");
static int view_batch_verdict(mirt_ctx* ctx, const char* fn, pt::ViewVerdict v, const pt::ViewDesc& d, uint32_t n_frames, uint32_t bad_frame) {
    switch (v) {
        case pt::VIEW_BATCH_TILE: return fail(ctx, MIRT_E_ARG, "%s: row tile [%u,+%u): a batch renders whole frames only (row0 0, nrows 0 or height)", fn, d.row0, d.nrows);
        case pt::VIEW_BATCH_NO_CAMERAS: return fail(ctx, MIRT_E_ARG, "%s: cameras is NULL with %u frames", fn, n_frames);
        case pt::VIEW_BATCH_CAMERA: return fail(ctx, MIRT_E_ARG, "%s: a component of eye, right, up or forward of the camera of frame %u is not finite", fn, bad_frame);
        case pt::VIEW_BATCH_RAYS: return fail(ctx, MIRT_E_ARG, "%s: %u frames of %u x %u x %u rays are more than 2^32 - 256 rays (the kernels index the batch's rays with 32 bits); render fewer frames per call", fn, n_frames, d.width, d.height, d.k * d.k);
        default: return view_verdict(ctx, fn, v, d);
    }
}
// The host array into the context's device table, in stream order.  *table: where the kernels read it.  Only growing the table waits for the
// stream (the one in place may still be read); it grows to twice the need, so a caller whose batches grow stalls a logarithmic number of times.
static int upload_cameras(mirt_ctx* ctx, const mirt_view_camera* cameras, uint32_t n_frames, const float** table) {
    const size_t bytes = (size_t)n_frames * sizeof(mirt_view_camera);
    if (ctx->camera_table_bytes < bytes) {
        if (ctx->camera_table) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(ctx->camera_table)); ctx->camera_table = nullptr; ctx->camera_table_bytes = 0; }
        HIPCHK(ctx, hipMalloc(&ctx->camera_table, 2 * bytes));
        ctx->camera_table_bytes = 2 * bytes;
    }
    pt::launch_viewCameras(ctx->stream, &cameras[0].eye[0], n_frames, (float*)ctx->camera_table);
    HIPCHK(ctx, hipGetLastError());
    *table = (const float*)ctx->camera_table;
    return MIRT_OK;
}
static pt::ViewBatchArgs view_batch_args(const pt::ViewDesc& d, const pt::ViewBatchPlan& plan, const float* table) {
    pt::ViewBatchArgs V;
    memset(&V, 0, sizeof V);
    static_cast<pt::ViewArgs&>(V) = view_args(d, plan.all);
    for (int c = 0; c < 3; ++c) V.eye[c] = V.right[c] = V.up[c] = V.forward[c] = 0.0f;   // not read: the table has the cameras
    V.row0 = 0u;
    V.cameras = table;
    V.frame_rows = plan.frame_rows;
    return V;
}

// mirt_render_view (guided false: seeds, radiance, pixel), mirt_view_guides (frame false: normal_hits, albedo_depth) and mirt_render_view_guided
// (all five): one list of checks, every one before anything is queued, then the launches.
// The frames of a batch: the host array and its length (mirt_render_view_batch, mirt_view_guides_batch, mirt_render_view_guided_batch); nullptr
// for the single calls
struct ViewBatch { const mirt_view_camera* cameras; uint32_t n_frames; };
static int render_view_impl(mirt_ctx* ctx, const char* fn, bool frame, bool guided, const mirt_pass_desc* d, const mirt_view_desc* vd, const ViewBatch* batch, mirt_buf* seeds,
                            mirt_buf* radiance, mirt_buf* pixel, mirt_buf* normal_hits, mirt_buf* albedo_depth) {
    ENTRY_PROLOGUE(ctx, fn);
    if (!d || d->struct_size != sizeof(mirt_pass_desc)) return fail(ctx, MIRT_E_ARG, "%s: descriptor size mismatch", fn);
    if (!vd || vd->struct_size != sizeof(mirt_view_desc)) return fail(ctx, MIRT_E_ARG, "%s: view descriptor size mismatch", fn);
    pt::ViewDesc v;
    memcpy(&v, vd, sizeof v);
    int rc;
    const bool nh = normal_hits != nullptr, ad = albedo_depth != nullptr;
    uint32_t bad_frame = 0;
    const pt::ViewCamera* const cams = batch ? (const pt::ViewCamera*)batch->cameras : nullptr;
    const pt::ViewVerdict verdict = batch    ? (!frame   ? pt::view_check_guides_batch(v, cams, batch->n_frames, nh, ad, &bad_frame)
                                                : guided ? pt::view_check_render_guided_batch(v, cams, batch->n_frames, seeds != nullptr, radiance != nullptr, pixel != nullptr, nh, ad, &bad_frame)
                                                         : pt::view_check_render_batch(v, cams, batch->n_frames, seeds != nullptr, radiance != nullptr, pixel != nullptr, &bad_frame))
                                    : !frame ? pt::view_check_guides(v, nh, ad)
                                    : guided ? pt::view_check_render_guided(v, seeds != nullptr, radiance != nullptr, pixel != nullptr, nh, ad)
                                             : pt::view_check_render(v, seeds != nullptr, radiance != nullptr, pixel != nullptr);
    if ((rc = batch ? view_batch_verdict(ctx, fn, verdict, v, batch->n_frames, bad_frame) : view_verdict(ctx, fn, verdict, v))) return rc;
    const pt::ViewBatchPlan bplan = batch ? pt::view_batch_plan(v, batch->n_frames) : pt::ViewBatchPlan();
    const pt::ViewPlan plan = batch ? bplan.all : pt::view_plan(v);   // the batch: the plan of the stacked image, the checks below on the whole batch buffers
    // the pass's own limits and rules for its arrays, as mirt_trace_radiance has them (the guides alone read no light)
    if ((rc = check_desc_arrays(ctx, fn, d, frame, "light/mesh"))) return rc;
    // everything given is written: the bytes the call touches of them, against each other's, the geometry's buffers and the material whole
    // (mirt_render_view's two messages are the ones it had before the guides: that call has none)
    const CallBuf io[5] = {{"seeds", seeds, plan.rays * 4}, {"radiance", radiance, plan.pixels * 16}, {"pixel", pixel, plan.pixels * 4},
                           {"normal_hits", normal_hits, plan.pixels * 16}, {"albedo_depth", albedo_depth, plan.pixels * 16}};
    if ((rc = check_call_buffers(ctx, fn, io, d, true,
                                 !frame   ? "%s: a guide's bytes meet a geometry buffer's or the material's"
                                 : guided ? "%s: the seeds', the radiance's, the pixel's or a guide's bytes meet a geometry buffer's or the material's"
                                          : "%s: the seeds', the radiance's or the pixel's bytes meet a geometry buffer's or the material's",
                                 !frame   ? "%s: normal_hits aliases albedo_depth"
                                 : guided ? "%s: seeds, radiance, pixel and the guides meet one another"
                                          : "%s: seeds, radiance and pixel meet one another"))) return rc;
    if (batch && !batch->n_frames) return MIRT_OK;   // no frames: nothing is queued, not even the geometry's preparation
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pt::FusedArgs A;
    memset(&A, 0, sizeof A);
    A.bounces = d->bounces;
    A.n_lights = frame ? d->n_lights : 0u;
    if ((rc = fill_sets(ctx, fn, d, A))) return rc;
    if ((rc = fill_shading(ctx, d, A, true))) return rc;
    const pt::ViewArgs V = view_args(v, plan);
    pt::ViewBatchArgs VB;
    memset(&VB, 0, sizeof VB);
    if (batch) {
        const float* table = nullptr;
        if ((rc = upload_cameras(ctx, batch->cameras, batch->n_frames, &table))) return rc;
        VB = view_batch_args(v, bplan, table);
    }
    void* const nhp = normal_hits ? normal_hits->ptr : nullptr;
    void* const adp = albedo_depth ? albedo_depth->ptr : nullptr;
    if (frame) {
        const bool accumulate = (v.flags & MIRT_VIEW_ACCUMULATE) != 0u;
        void* const rp = radiance ? radiance->ptr : nullptr;
        void* const pp = pixel ? pixel->ptr : nullptr;
        const bool in_pass = guided && (batch ? pt::view_batch_guides_in_pass(plan.rpp, pt::fused_has_grids(A), guided_view_enabled())
                                              : pt::view_guides_in_pass(plan.rpp, pt::fused_has_grids(A), guided_view_enabled()));
        pt::FusedArgs F = A;
        if (in_pass) { F.guide_nh = nhp; F.guide_ad = adp; }
        rc = queue_pair(ctx, ctx->view_mask, A, plan.mask_words, 256u, [&](bool fast, uint32_t* mask_out, const uint32_t* mask_in) {   // a bit is a block of 256 rays
            if (batch) pt::launch_viewPassBatch(ctx->stream, F, VB, fast, accumulate, (int32_t*)seeds->ptr, rp, pp, v.tone, mask_out, mask_in);
            else pt::launch_viewPass(ctx->stream, F, V, fast, accumulate, (int32_t*)seeds->ptr, rp, pp, v.tone, mask_out, mask_in);
        });
        if (rc) return rc;
        if (in_pass) ctx->guided_views++;
        else if (guided && (rc = batch ? queue_view_guides_batch(ctx, A, VB, bplan, nhp, adp) : queue_view_guides(ctx, A, V, plan, nhp, adp))) return rc;   // everywhere else: exactly what mirt_view_guides (_batch) queues
    } else if ((rc = batch ? queue_view_guides_batch(ctx, A, VB, bplan, nhp, adp) : queue_view_guides(ctx, A, V, plan, nhp, adp))) return rc;
    return finish_call(ctx, io, 5);
}

int mirt_render_view(mirt_ctx* ctx, const mirt_pass_desc* d, const mirt_view_desc* vd, mirt_buf* seeds, mirt_buf* radiance, mirt_buf* pixel) try {
    return render_view_impl(ctx, "mirt_render_view", true, false, d, vd, nullptr, seeds, radiance, pixel, nullptr, nullptr);
} MIRT_CATCH("mirt_render_view", return MIRT_E_DEVICE)

int mirt_view_rays_batch(mirt_ctx* ctx, const mirt_view_desc* vd, const mirt_view_camera* cameras, uint32_t n_frames, mirt_buf* rays) try {
    const char* const fn = "mirt_view_rays_batch";
    ENTRY_PROLOGUE(ctx, fn);
    if (!vd || vd->struct_size != sizeof(mirt_view_desc)) return fail(ctx, MIRT_E_ARG, "%s: view descriptor size mismatch", fn);
    pt::ViewDesc d;
    memcpy(&d, vd, sizeof d);
    int rc;
    uint32_t bad = 0;
    const pt::ViewVerdict verdict = pt::view_check_batch(d, (const pt::ViewCamera*)cameras, n_frames, &bad);
    if ((rc = view_batch_verdict(ctx, fn, verdict, d, n_frames, bad))) return rc;
    const pt::ViewBatchPlan plan = pt::view_batch_plan(d, n_frames);
    if (!rays) return fail(ctx, MIRT_E_HANDLE, "%s: rays is NULL", fn);
    if ((rc = need(ctx, "mirt_view_rays_batch rays", rays, plan.all.rays * 32))) return rc;
    if (!n_frames) return MIRT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const float* table = nullptr;
    if ((rc = upload_cameras(ctx, cameras, n_frames, &table))) return rc;
    pt::launch_viewRaysBatch(ctx->stream, view_batch_args(d, plan, table), rays->ptr);
    HIPCHK(ctx, hipGetLastError());
    rays->version++;
    return MIRT_OK;
} MIRT_CATCH("mirt_view_rays_batch", return MIRT_E_DEVICE)

// The frames of n_frames cameras: mirt_render_view's list of checks on the whole batch buffers, its fills and its pair, with the batch's verdicts,
// plan and kernel instances (render_view_impl).
int mirt_render_view_batch(mirt_ctx* ctx, const mirt_pass_desc* d, const mirt_view_desc* vd, const mirt_view_camera* cameras, uint32_t n_frames, mirt_buf* seeds,
                           mirt_buf* radiance, mirt_buf* pixel) try {
    const ViewBatch batch = {cameras, n_frames};
    return render_view_impl(ctx, "mirt_render_view_batch", true, false, d, vd, &batch, seeds, radiance, pixel, nullptr, nullptr);
} MIRT_CATCH("mirt_render_view_batch", return MIRT_E_DEVICE)

// First-hit guides of a view camera's tile (pt_kernels_rays.hip k_viewGuides): one launch -- or the optimistic / exact pair, per pixel -- of one
// lane per pixel.  Nothing but the two outputs is written.
int mirt_view_guides(mirt_ctx* ctx, const mirt_pass_desc* d, const mirt_view_desc* vd, mirt_buf* normal_hits, mirt_buf* albedo_depth) try {
    return render_view_impl(ctx, "mirt_view_guides", false, true, d, vd, nullptr, nullptr, nullptr, nullptr, normal_hits, albedo_depth);
} MIRT_CATCH("mirt_view_guides", return MIRT_E_DEVICE)

// The frame and its guides in one call: where a pixel's samples are consecutive lanes of one wave (pt_view_plan.hpp view_guides_in_pass) the
// frame's own launches write the guides (k_viewPass GUIDES), elsewhere the guide launches follow.
int mirt_render_view_guided(mirt_ctx* ctx, const mirt_pass_desc* d, const mirt_view_desc* vd, mirt_buf* seeds, mirt_buf* radiance, mirt_buf* pixel, mirt_buf* normal_hits,
                            mirt_buf* albedo_depth) try {
    return render_view_impl(ctx, "mirt_render_view_guided", true, true, d, vd, nullptr, seeds, radiance, pixel, normal_hits, albedo_depth);
} MIRT_CATCH("mirt_render_view_guided", return MIRT_E_DEVICE)

// The guides of n_frames cameras' frames, alone and from the frames' launch: mirt_view_guides' and mirt_render_view_guided's lists of checks on the
// whole batch buffers behind the batch's own, and the batch's kernel instances (render_view_impl)
int mirt_view_guides_batch(mirt_ctx* ctx, const mirt_pass_desc* d, const mirt_view_desc* vd, const mirt_view_camera* cameras, uint32_t n_frames, mirt_buf* normal_hits,
                           mirt_buf* albedo_depth) try {
    const ViewBatch batch = {cameras, n_frames};
    return render_view_impl(ctx, "mirt_view_guides_batch", false, true, d, vd, &batch, nullptr, nullptr, nullptr, normal_hits, albedo_depth);
} MIRT_CATCH("mirt_view_guides_batch", return MIRT_E_DEVICE)

int mirt_render_view_guided_batch(mirt_ctx* ctx, const mirt_pass_desc* d, const mirt_view_desc* vd, const mirt_view_camera* cameras, uint32_t n_frames, mirt_buf* seeds,
                                  mirt_buf* radiance, mirt_buf* pixel, mirt_buf* normal_hits, mirt_buf* albedo_depth) try {
    const ViewBatch batch = {cameras, n_frames};
    return render_view_impl(ctx, "mirt_render_view_guided_batch", true, true, d, vd, &batch, seeds, radiance, pixel, normal_hits, albedo_depth);
} MIRT_CATCH("mirt_render_view_guided_batch", return MIRT_E_DEVICE)

int mirt_ctx_guided_views(mirt_ctx* ctx, uint64_t* count) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_ctx_guided_views: unknown context");
    if (!count) return fail(ctx, MIRT_E_ARG, "mirt_ctx_guided_views: null output");
    *count = ctx->guided_views;
    return MIRT_OK;
} MIRT_CATCH("mirt_ctx_guided_views", return MIRT_E_DEVICE)

// Ambient occlusion of a view camera's tile (pt_kernels_rays.hip k_viewAo): mirt_view_guides's checks without the material, mirt_render_ao's own
// (pt_view_plan.hpp view_check_ao), then one launch -- or the optimistic / exact pair, per pixel -- of one lane per pixel.  Every check comes
// before anything is queued; nothing but ao_out is written.
static_assert(sizeof(pt::ViewAoDesc) == sizeof(mirt_ao_desc) && offsetof(pt::ViewAoDesc, samples) == offsetof(mirt_ao_desc, samples) &&
              offsetof(pt::ViewAoDesc, radius) == offsetof(mirt_ao_desc, radius) && offsetof(pt::ViewAoDesc, bias) == offsetof(mirt_ao_desc, bias) &&
              pt::kViewAoMaxSamples == MIRT_AO_MAX_SAMPLES, "pt_view_plan.hpp restates the header's AO descriptor");
int mirt_view_ao(mirt_ctx* ctx, const mirt_pass_desc* d, const mirt_view_desc* vd, const mirt_ao_desc* ao, mirt_buf* seeds, mirt_buf* ao_out) try {
    const char* const fn = "mirt_view_ao";
    ENTRY_PROLOGUE(ctx, fn);
    if (!d || d->struct_size != sizeof(mirt_pass_desc)) return fail(ctx, MIRT_E_ARG, "%s: descriptor size mismatch", fn);
    if (!vd || vd->struct_size != sizeof(mirt_view_desc)) return fail(ctx, MIRT_E_ARG, "%s: view descriptor size mismatch", fn);
    if (!ao || ao->struct_size != sizeof(mirt_ao_desc)) return fail(ctx, MIRT_E_ARG, "%s: AO descriptor size mismatch", fn);
    pt::ViewDesc v;
    memcpy(&v, vd, sizeof v);
    pt::ViewAoDesc a;
    memcpy(&a, ao, sizeof a);
    int rc;
    if ((rc = view_verdict(ctx, fn, pt::view_check_ao(v, a, seeds != nullptr, ao_out != nullptr), v))) return rc;
    const pt::ViewPlan plan = pt::view_plan(v);
    if ((rc = check_desc_arrays(ctx, fn, d, false, "mesh"))) return rc;
    // the output is read by nobody and no input is written: the bytes the call writes, against the seeds' and the geometry's buffers whole
    const CallBuf io[2] = {{"seeds", seeds, plan.rays * 4, BUF_IN_WHOLE}, {"ao_out", ao_out, plan.pixels * 8}};
    if ((rc = check_call_buffers(ctx, fn, io, d, false, "%s: ao_out's bytes meet the seeds' or a geometry buffer's", nullptr))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pt::FusedArgs A;
    memset(&A, 0, sizeof A);
    if ((rc = fill_sets(ctx, fn, d, A))) return rc;
    const pt::ViewArgs V = view_args(v, plan);
    const pt::ViewGuidesPlan g = pt::view_guides_plan(plan);
    const int32_t* const sp = (const int32_t*)seeds->ptr;
    rc = queue_pair(ctx, ctx->view_ao_mask, A, g.mask_words, 1u, [&](bool fast, uint32_t* mask_out, const uint32_t* mask_in) {
        pt::launch_viewAo(ctx->stream, A, V, g.blocks, fast, a.samples, a.radius, a.bias, sp, ao_out->ptr, mask_out, mask_in);
    });
    return rc ? rc : finish_call(ctx, io, 2);
} MIRT_CATCH("mirt_view_ao", return MIRT_E_DEVICE)

// Ambient occlusion of n_frames cameras' frames (k_viewAoBatch): mirt_view_ao's shape on the whole batch buffers, with the batch's verdicts first,
// the camera table and the plan of the stacked image.  A descriptor of another size is read no further than its first word.
int mirt_view_ao_batch(mirt_ctx* ctx, const mirt_pass_desc* d, const mirt_view_desc* vd, const mirt_view_camera* cameras, uint32_t n_frames, const mirt_ao_desc* ao,
                       mirt_buf* seeds, mirt_buf* ao_out) try {
    const char* const fn = "mirt_view_ao_batch";
    ENTRY_PROLOGUE(ctx, fn);
    if (!d || d->struct_size != sizeof(mirt_pass_desc)) return fail(ctx, MIRT_E_ARG, "%s: descriptor size mismatch", fn);
    if (!vd || vd->struct_size != sizeof(mirt_view_desc)) return fail(ctx, MIRT_E_ARG, "%s: view descriptor size mismatch", fn);
    pt::ViewDesc v;
    memcpy(&v, vd, sizeof v);
    pt::ViewAoDesc a;
    memset(&a, 0, sizeof a);
    if (ao && ao->struct_size == sizeof(mirt_ao_desc)) memcpy(&a, ao, sizeof a);
    int rc;
    uint32_t bad_frame = 0;
    const pt::ViewVerdict verdict = pt::view_check_ao_batch(v, (const pt::ViewCamera*)cameras, n_frames, a, seeds != nullptr, ao_out != nullptr, &bad_frame);
    if ((rc = view_batch_verdict(ctx, fn, verdict, v, n_frames, bad_frame))) return rc;
    const pt::ViewBatchPlan bplan = pt::view_batch_plan(v, n_frames);
    if ((rc = check_desc_arrays(ctx, fn, d, false, "mesh"))) return rc;
    const CallBuf io[2] = {{"seeds", seeds, bplan.all.rays * 4, BUF_IN_WHOLE}, {"ao_out", ao_out, bplan.all.pixels * 8}};
    if ((rc = check_call_buffers(ctx, fn, io, d, false, "%s: ao_out's bytes meet the seeds' or a geometry buffer's", nullptr))) return rc;
    if (!n_frames) return MIRT_OK;   // no frames: nothing is queued, and the counter of the last call stays
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pt::FusedArgs A;
    memset(&A, 0, sizeof A);
    if ((rc = fill_sets(ctx, fn, d, A))) return rc;
    const float* table = nullptr;
    if ((rc = upload_cameras(ctx, cameras, n_frames, &table))) return rc;
    const pt::ViewBatchArgs VB = view_batch_args(v, bplan, table);
    const pt::ViewGuidesPlan g = pt::view_batch_pixel_plan(bplan);
    const int32_t* const sp = (const int32_t*)seeds->ptr;
    rc = queue_pair(ctx, ctx->view_ao_mask, A, g.mask_words, 1u, [&](bool fast, uint32_t* mask_out, const uint32_t* mask_in) {
        pt::launch_viewAoBatch(ctx->stream, A, VB, g.blocks, fast, a.samples, a.radius, a.bias, sp, ao_out->ptr, mask_out, mask_in);
    });
    return rc ? rc : finish_call(ctx, io, 2);
} MIRT_CATCH("mirt_view_ao_batch", return MIRT_E_DEVICE)

int mirt_view_ao_deferred(mirt_ctx* ctx, uint64_t* pixels) try {
    ENTRY_PROLOGUE(ctx, "mirt_view_ao_deferred");
    return count_deferred(ctx, "mirt_view_ao_deferred", ctx->view_ao_mask, pixels);
} MIRT_CATCH("mirt_view_ao_deferred", return MIRT_E_DEVICE)

int mirt_view_deferred(mirt_ctx* ctx, uint64_t* rays) try {
    ENTRY_PROLOGUE(ctx, "mirt_view_deferred");
    return count_deferred(ctx, "mirt_view_deferred", ctx->view_mask, rays);
} MIRT_CATCH("mirt_view_deferred", return MIRT_E_DEVICE)

// ---- the post-process stage: mirt_filter_atrous and mirt_upsample_guided.  The argument rules they share are pt_post_check.hpp's (host-only,
// CPU-tested); here are those rules' messages, `fn` being the entry point's name.
static_assert(pt::kPostMaxNormalPowerLog2 == MIRT_FILTER_MAX_NORMAL_POWER_LOG2, "pt_post_check.hpp restates the header's limit");

static int post_check_extent(mirt_ctx* ctx, const char* fn, uint32_t w, uint32_t h) {
    const pt::PostExtent e = pt::post_extent(w, h);
    if (e == pt::POST_EXTENT_EMPTY) return fail(ctx, MIRT_E_ARG, "%s: empty image", fn);
    if (e == pt::POST_EXTENT_TOO_LARGE) return fail(ctx, MIRT_E_ARG, "%s: %ux%u is more than 65535 pixels a side", fn, w, h);
    return MIRT_OK;
}
static int post_check_terms(mirt_ctx* ctx, const char* fn, uint32_t npow, float tone) {
    if (!pt::post_normal_power_ok(npow)) return fail(ctx, MIRT_E_ARG, "%s: normal_power_log2 %u > %u", fn, npow, MIRT_FILTER_MAX_NORMAL_POWER_LOG2);
    if (!pt::post_finite_positive(tone)) return fail(ctx, MIRT_E_ARG, "%s: tone %g is not a finite positive factor", fn, (double)tone);
    return MIRT_OK;
}
// b: the N - 2 inputs, then the two outputs, `first` (the first one's name) and pixel.  One of the outputs is given; every buffer given is live,
// this context's and large enough; an output is read by nobody and no input is written: the same handle, or (wrapped memory) the same bytes,
// twice is refused.  Nothing is formatted or allocated unless a check fails: a caller that times the call times this too.
extern "C++" {
template <size_t N>
int post_check_buffers(mirt_ctx* ctx, const char* fn, const char* first, const CallBuf (&b)[N]) {
    if (!b[N - 2].buf && !b[N - 1].buf) return fail(ctx, MIRT_E_ARG, "%s: %s and pixel are both NULL (either may be, not both)", fn, first);
    pt::PostRange r[N];
    for (size_t i = 0; i < N; ++i) {
        r[i] = {0, b[i].bytes, i < N - 2 || b[i].buf != nullptr};
        if (!r[i].present) continue;
        if (int rc = need(ctx, b[i].label, b[i].buf, b[i].bytes)) return rc;
        r[i].addr = (uint64_t)(uintptr_t)b[i].buf->ptr;
    }
    const pt::PostAlias alias = pt::post_alias(r, N - 2, r + N - 2, 2);
    if (alias == pt::POST_ALIAS_OUTPUT_INPUT) return fail(ctx, MIRT_E_ARG, "%s: an output aliases an input", fn);
    if (alias == pt::POST_ALIAS_OUTPUTS) return fail(ctx, MIRT_E_ARG, "%s: %s aliases pixel", fn, first);
    return MIRT_OK;
}
}  // extern "C++"

// The a-trous filter (pt_kernels_filter.hip; defined in include/mirt.h): every check first, then the prepare launch and one launch per iteration,
// the last of which writes the outputs.  The two working images and the prepared guide are three float4 arrays of the context's scratch buffer,
// asked for ONCE (growing the buffer frees the old one: pt_pass_plan.hpp).
int mirt_filter_atrous(mirt_ctx* ctx, const mirt_filter_desc* d) try {
    static const char fn[] = "mirt_filter_atrous";
    ENTRY_PROLOGUE(ctx, "mirt_filter_atrous");
    if (!d || d->struct_size != sizeof(mirt_filter_desc)) return fail(ctx, MIRT_E_ARG, "mirt_filter_atrous: descriptor size mismatch");
    int rc;
    if ((rc = post_check_extent(ctx, fn, d->width, d->height))) return rc;
    if (d->iterations > MIRT_FILTER_MAX_ITERATIONS) return fail(ctx, MIRT_E_ARG, "mirt_filter_atrous: %u iterations > %u", d->iterations, MIRT_FILTER_MAX_ITERATIONS);
    if ((rc = post_check_terms(ctx, fn, d->normal_power_log2, d->tone))) return rc;
    const uint32_t both = MIRT_FILTER_DIRECT | MIRT_FILTER_TILED;
    if ((d->flags & ~(MIRT_FILTER_DEMODULATE | both)) || (d->flags & both) == both) return fail(ctx, MIRT_E_ARG, "mirt_filter_atrous: unknown flags 0x%x (or both structures forced)", d->flags);
    const uint64_t npix = (uint64_t)d->width * d->height;
    const CallBuf b[5] = {{"mirt_filter_atrous radiance", d->radiance, npix * 16}, {"mirt_filter_atrous normal_hits", d->normal_hits, npix * 16}, {"mirt_filter_atrous albedo_depth", d->albedo_depth, npix * 16},
                          {"mirt_filter_atrous filtered", d->filtered, npix * 16}, {"mirt_filter_atrous pixel", d->pixel, npix * 4}};
    if ((rc = post_check_buffers(ctx, fn, "filtered", b))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pt::FilterArgs A;
    memset(&A, 0, sizeof A);
    A.width = d->width; A.height = d->height;
    A.demodulate = (d->flags & MIRT_FILTER_DEMODULATE) ? 1u : 0u;
    A.npow = d->normal_power_log2;
    A.depth_on = pt::post_finite_positive(d->sigma_depth);
    A.colour_on = pt::post_finite_positive(d->sigma_colour);
    A.tone = d->tone; A.sigma_depth = d->sigma_depth;
    A.radiance = d->radiance->ptr; A.normal_hits = d->normal_hits->ptr; A.albedo_depth = d->albedo_depth->ptr;
    A.filtered = d->filtered ? d->filtered->ptr : nullptr;
    A.pixel = d->pixel ? d->pixel->ptr : nullptr;
    if (d->iterations) {
        const size_t plane = (size_t)npix * 16;
        if ((rc = ensure_scratch(ctx, 3 * plane))) return rc;
        char* const scratch = (char*)ctx->scratch;
        A.work[0] = scratch; A.work[1] = scratch + plane; A.guide = scratch + 2 * plane;
    }
    pt::launch_filterPrepare(ctx->stream, A, d->iterations == 0u);
    for (uint32_t i = 0; i < d->iterations; ++i) {
        // inv_i = 1 / (k_i * k_i), k_i = sigma_colour * 2^-i: three IEEE fp32 operations of the host, each rounded on its own
        volatile float k = d->sigma_colour * std::ldexp(1.0f, -(int)i);
        volatile float kk = k * k;
        volatile float inv = 1.0f / kk;
        const bool tiled = (d->flags & both) ? (d->flags & MIRT_FILTER_TILED) != 0u : (pt::kFilterTiledSteps >> i & 1u) != 0u;
        pt::launch_filterStep(ctx->stream, A, i & 1u, i, A.colour_on ? inv : 0.0f, i + 1u == d->iterations, tiled);
    }
    return finish_call(ctx, b + 3, 2);
} MIRT_CATCH("mirt_filter_atrous", return MIRT_E_DEVICE)

// Guide-driven upsampling (pt_kernels_upsample.hip; defined in include/mirt.h): every check first, then one launch.  No working memory.
int mirt_upsample_guided(mirt_ctx* ctx, const mirt_upsample_desc* d) try {
    static const char fn[] = "mirt_upsample_guided";
    ENTRY_PROLOGUE(ctx, "mirt_upsample_guided");
    if (!d || d->struct_size != sizeof(mirt_upsample_desc)) return fail(ctx, MIRT_E_ARG, "mirt_upsample_guided: descriptor size mismatch");
    int rc;
    if ((rc = post_check_extent(ctx, fn, d->width, d->height))) return rc;
    if (!pt::upsample_factor_ok(d->factor))
        return fail(ctx, MIRT_E_ARG, "mirt_upsample_guided: factor %u is outside %u .. %u", d->factor, MIRT_UPSAMPLE_MIN_FACTOR, MIRT_UPSAMPLE_MAX_FACTOR);
    const uint32_t wl = pt::upsample_low_extent(d->width, d->factor), hl = pt::upsample_low_extent(d->height, d->factor);
    if (!wl || !hl)
        return fail(ctx, MIRT_E_ARG, "mirt_upsample_guided: %ux%u is not a multiple of factor %u (the two images would not show the same frustum)", d->width, d->height, d->factor);
    if ((rc = post_check_terms(ctx, fn, d->normal_power_log2, d->tone))) return rc;
    if (d->flags & ~MIRT_UPSAMPLE_DEMODULATE) return fail(ctx, MIRT_E_ARG, "mirt_upsample_guided: unknown flags 0x%x", d->flags);
    const uint64_t npix = (uint64_t)d->width * d->height, nlo = (uint64_t)wl * hl;
    const CallBuf b[7] = {{"mirt_upsample_guided radiance_lo", d->radiance_lo, nlo * 16}, {"mirt_upsample_guided normal_hits_lo", d->normal_hits_lo, nlo * 16}, {"mirt_upsample_guided albedo_depth_lo", d->albedo_depth_lo, nlo * 16},
                          {"mirt_upsample_guided normal_hits", d->normal_hits, npix * 16}, {"mirt_upsample_guided albedo_depth", d->albedo_depth, npix * 16},
                          {"mirt_upsample_guided upsampled", d->upsampled, npix * 16}, {"mirt_upsample_guided pixel", d->pixel, npix * 4}};
    if ((rc = post_check_buffers(ctx, fn, "upsampled", b))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pt::UpsampleArgs A;
    memset(&A, 0, sizeof A);
    A.width = d->width; A.height = d->height; A.factor = d->factor;
    A.demodulate = (d->flags & MIRT_UPSAMPLE_DEMODULATE) ? 1u : 0u;
    A.npow = d->normal_power_log2;
    A.depth_on = pt::post_finite_positive(d->sigma_depth);
    A.tone = d->tone; A.sigma_depth = d->sigma_depth;
    A.radiance_lo = d->radiance_lo->ptr; A.normal_hits_lo = d->normal_hits_lo->ptr; A.albedo_depth_lo = d->albedo_depth_lo->ptr;
    A.normal_hits = d->normal_hits->ptr; A.albedo_depth = d->albedo_depth->ptr;
    A.upsampled = d->upsampled ? d->upsampled->ptr : nullptr;
    A.pixel = d->pixel ? d->pixel->ptr : nullptr;
    pt::launch_upsample(ctx->stream, A);
    return finish_call(ctx, b + 5, 2);
} MIRT_CATCH("mirt_upsample_guided", return MIRT_E_DEVICE)

// ---- the post-process stage in row tiles: mirt_filter_atrous_rows, mirt_upsample_guided_rows and the halo exchange between them, mirt_exchange_rows.
// The row arithmetic and the rules of the rows are pt_rows_plan.hpp's (host-only, CPU-tested); here are their messages.
static_assert(pt::kRowsMaxIterations == MIRT_FILTER_MAX_ITERATIONS, "pt_rows_plan.hpp restates the header's limit");

void mirt_filter_window_rows(uint32_t image_height, uint32_t row0, uint32_t nrows, uint32_t iterations, uint32_t* win_row0, uint32_t* win_nrows) try {
    const pt::RowRange w = pt::filter_window(image_height, row0, nrows, iterations);
    if (win_row0) *win_row0 = w.row0;
    if (win_nrows) *win_nrows = w.nrows;
} MIRT_CATCH("mirt_filter_window_rows", return)

void mirt_upsample_low_rows(uint32_t height, uint32_t factor, uint32_t row0, uint32_t nrows, uint32_t* lo_row0, uint32_t* lo_nrows) try {
    const pt::RowRange w = pt::upsample_low_window(height, factor, row0, nrows);
    if (lo_row0) *lo_row0 = w.row0;
    if (lo_nrows) *lo_nrows = w.nrows;
} MIRT_CATCH("mirt_upsample_low_rows", return)

static int rows_verdict(mirt_ctx* ctx, const char* fn, pt::RowsVerdict v, const char* window, uint32_t w0, uint32_t wn, uint32_t row0, uint32_t nrows, const pt::RowRange& need) {
    if (v == pt::ROWS_EMPTY) return fail(ctx, MIRT_E_ARG, "%s: no rows asked for, or an empty %s", fn, window);
    if (v == pt::ROWS_OUTSIDE_IMAGE) return fail(ctx, MIRT_E_ARG, "%s: rows [%u, +%u) or the %s [%u, +%u) reach outside the image", fn, row0, nrows, window, w0, wn);
    if (v == pt::ROWS_WINDOW_SHORT)
        return fail(ctx, MIRT_E_ARG, "%s: the %s [%u, +%u) does not contain [%u, +%u), the rows that rows [%u, +%u) depend on", fn, window, w0, wn, need.row0, need.nrows, row0, nrows);
    return MIRT_OK;
}

// The a-trous filter of rows [row0, row0 + nrows) from a window of the image (defined in include/mirt.h): mirt_filter_atrous's checks and launches
// with the window as the image the kernels see; every launch computes its band of the window alone (pt_rows_plan.hpp's filter_band), the last one
// the own rows.  MIRT_FILTER_ROWS_BAND=0 (a measurement switch: profiles/post_rows_bench.py): every launch but the last computes the whole window.
int mirt_filter_atrous_rows(mirt_ctx* ctx, const mirt_filter_desc* d, uint32_t image_height, uint32_t win_row0, uint32_t row0, uint32_t nrows) try {
    static const char fn[] = "mirt_filter_atrous_rows";
    ENTRY_PROLOGUE(ctx, "mirt_filter_atrous_rows");
    if (!d || d->struct_size != sizeof(mirt_filter_desc)) return fail(ctx, MIRT_E_ARG, "mirt_filter_atrous_rows: descriptor size mismatch");
    int rc;
    if ((rc = post_check_extent(ctx, fn, d->width, image_height))) return rc;
    if (d->iterations > MIRT_FILTER_MAX_ITERATIONS) return fail(ctx, MIRT_E_ARG, "mirt_filter_atrous_rows: %u iterations > %u", d->iterations, MIRT_FILTER_MAX_ITERATIONS);
    if ((rc = post_check_terms(ctx, fn, d->normal_power_log2, d->tone))) return rc;
    const uint32_t both = MIRT_FILTER_DIRECT | MIRT_FILTER_TILED;
    if ((d->flags & ~(MIRT_FILTER_DEMODULATE | both)) || (d->flags & both) == both) return fail(ctx, MIRT_E_ARG, "mirt_filter_atrous_rows: unknown flags 0x%x (or both structures forced)", d->flags);
    const uint32_t win_nrows = d->height;
    if ((rc = rows_verdict(ctx, fn, pt::filter_rows_check(image_height, win_row0, win_nrows, row0, nrows, d->iterations), "window", win_row0, win_nrows, row0, nrows,
                           pt::filter_window(image_height, row0, nrows, d->iterations)))) return rc;
    const uint64_t nwin = (uint64_t)d->width * win_nrows, nown = (uint64_t)d->width * nrows;
    const CallBuf b[5] = {{"mirt_filter_atrous_rows radiance", d->radiance, nwin * 16}, {"mirt_filter_atrous_rows normal_hits", d->normal_hits, nwin * 16}, {"mirt_filter_atrous_rows albedo_depth", d->albedo_depth, nwin * 16},
                          {"mirt_filter_atrous_rows filtered", d->filtered, nown * 16}, {"mirt_filter_atrous_rows pixel", d->pixel, nown * 4}};
    if ((rc = post_check_buffers(ctx, fn, "filtered", b))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pt::FilterRowsArgs A;
    memset(&A, 0, sizeof A);
    A.width = d->width; A.height = win_nrows;
    A.demodulate = (d->flags & MIRT_FILTER_DEMODULATE) ? 1u : 0u;
    A.npow = d->normal_power_log2;
    A.depth_on = pt::post_finite_positive(d->sigma_depth);
    A.colour_on = pt::post_finite_positive(d->sigma_colour);
    A.tone = d->tone; A.sigma_depth = d->sigma_depth;
    A.radiance = d->radiance->ptr; A.normal_hits = d->normal_hits->ptr; A.albedo_depth = d->albedo_depth->ptr;
    A.filtered = d->filtered ? d->filtered->ptr : nullptr;
    A.pixel = d->pixel ? d->pixel->ptr : nullptr;
    if (d->iterations) {
        const size_t plane = (size_t)nwin * 16;
        if ((rc = ensure_scratch(ctx, 3 * plane))) return rc;
        char* const scratch = (char*)ctx->scratch;
        A.work[0] = scratch; A.work[1] = scratch + plane; A.guide = scratch + 2 * plane;
    }
    const char* const be = getenv("MIRT_FILTER_ROWS_BAND");
    const bool shrink = !(be && be[0] == '0');
    // the band of launch i (the prepare: i == iterations), in rows of the window
    const auto band = [&](uint32_t i) {
        const bool last = i + 1u == d->iterations || d->iterations == 0u;
        const pt::RowRange r = shrink || last ? pt::filter_band(win_row0, win_nrows, row0, nrows, d->iterations, i) : pt::RowRange{win_row0, win_nrows};
        A.band_row0 = r.row0 - win_row0; A.band_nrows = r.nrows;
    };
    band(d->iterations);
    pt::launch_filterPrepareRows(ctx->stream, A, d->iterations == 0u);
    for (uint32_t i = 0; i < d->iterations; ++i) {
        // inv_i as in mirt_filter_atrous: three IEEE fp32 operations of the host, each rounded on its own
        volatile float k = d->sigma_colour * std::ldexp(1.0f, -(int)i);
        volatile float kk = k * k;
        volatile float inv = 1.0f / kk;
        const bool tiled = (d->flags & both) ? (d->flags & MIRT_FILTER_TILED) != 0u : (pt::kFilterTiledSteps >> i & 1u) != 0u;
        band(i);
        pt::launch_filterStepRows(ctx->stream, A, i & 1u, i, A.colour_on ? inv : 0.0f, i + 1u == d->iterations, tiled);
    }
    return finish_call(ctx, b + 3, 2);
} MIRT_CATCH("mirt_filter_atrous_rows", return MIRT_E_DEVICE)

// Guide-driven upsampling of high rows [row0, row0 + nrows) (defined in include/mirt.h): mirt_upsample_guided's checks on the whole image, the rule
// of the low rows, then one launch over the band.
int mirt_upsample_guided_rows(mirt_ctx* ctx, const mirt_upsample_desc* d, uint32_t row0, uint32_t nrows, uint32_t lo_row0, uint32_t lo_nrows) try {
    static const char fn[] = "mirt_upsample_guided_rows";
    ENTRY_PROLOGUE(ctx, "mirt_upsample_guided_rows");
    if (!d || d->struct_size != sizeof(mirt_upsample_desc)) return fail(ctx, MIRT_E_ARG, "mirt_upsample_guided_rows: descriptor size mismatch");
    int rc;
    if ((rc = post_check_extent(ctx, fn, d->width, d->height))) return rc;
    if (!pt::upsample_factor_ok(d->factor))
        return fail(ctx, MIRT_E_ARG, "mirt_upsample_guided_rows: factor %u is outside %u .. %u", d->factor, MIRT_UPSAMPLE_MIN_FACTOR, MIRT_UPSAMPLE_MAX_FACTOR);
    const uint32_t wl = pt::upsample_low_extent(d->width, d->factor), hl = pt::upsample_low_extent(d->height, d->factor);
    if (!wl || !hl)
        return fail(ctx, MIRT_E_ARG, "mirt_upsample_guided_rows: %ux%u is not a multiple of factor %u (the two images would not show the same frustum)", d->width, d->height, d->factor);
    if ((rc = post_check_terms(ctx, fn, d->normal_power_log2, d->tone))) return rc;
    if (d->flags & ~MIRT_UPSAMPLE_DEMODULATE) return fail(ctx, MIRT_E_ARG, "mirt_upsample_guided_rows: unknown flags 0x%x", d->flags);
    if ((rc = rows_verdict(ctx, fn, pt::upsample_rows_check(d->height, d->factor, row0, nrows, lo_row0, lo_nrows), "low rows", lo_row0, lo_nrows, row0, nrows,
                           pt::upsample_low_window(d->height, d->factor, row0, nrows)))) return rc;
    const uint64_t npix = (uint64_t)d->width * nrows, nlo = (uint64_t)wl * lo_nrows;
    const CallBuf b[7] = {{"mirt_upsample_guided_rows radiance_lo", d->radiance_lo, nlo * 16}, {"mirt_upsample_guided_rows normal_hits_lo", d->normal_hits_lo, nlo * 16}, {"mirt_upsample_guided_rows albedo_depth_lo", d->albedo_depth_lo, nlo * 16},
                          {"mirt_upsample_guided_rows normal_hits", d->normal_hits, npix * 16}, {"mirt_upsample_guided_rows albedo_depth", d->albedo_depth, npix * 16},
                          {"mirt_upsample_guided_rows upsampled", d->upsampled, npix * 16}, {"mirt_upsample_guided_rows pixel", d->pixel, npix * 4}};
    if ((rc = post_check_buffers(ctx, fn, "upsampled", b))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pt::UpsampleRowsArgs A;
    memset(&A, 0, sizeof A);
    A.width = d->width; A.height = d->height; A.factor = d->factor;
    A.demodulate = (d->flags & MIRT_UPSAMPLE_DEMODULATE) ? 1u : 0u;
    A.npow = d->normal_power_log2;
    A.depth_on = pt::post_finite_positive(d->sigma_depth);
    A.tone = d->tone; A.sigma_depth = d->sigma_depth;
    A.radiance_lo = d->radiance_lo->ptr; A.normal_hits_lo = d->normal_hits_lo->ptr; A.albedo_depth_lo = d->albedo_depth_lo->ptr;
    A.normal_hits = d->normal_hits->ptr; A.albedo_depth = d->albedo_depth->ptr;
    A.upsampled = d->upsampled ? d->upsampled->ptr : nullptr;
    A.pixel = d->pixel ? d->pixel->ptr : nullptr;
    A.row0 = row0; A.nrows = nrows; A.lo_row0 = lo_row0;
    pt::launch_upsampleRows(ctx->stream, A);
    return finish_call(ctx, b + 5, 2);
} MIRT_CATCH("mirt_upsample_guided_rows", return MIRT_E_DEVICE)

// The halo exchange (defined in include/mirt.h): every check, then the plan of pt_rows_plan.hpp as copies on the destinations' streams, between
// events that order them after the sources' work and the sources' next work after them.
namespace {
struct EventSet {   // events of one call, destroyed when it returns: the runtime releases each once the work queued on it has completed
    std::vector<hipEvent_t> ev;
    explicit EventSet(size_t n) : ev(n, nullptr) {}
    ~EventSet() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};
}  // namespace
int mirt_exchange_rows(mirt_group* g, mirt_buf* const* src, const uint32_t* src_row0, const uint32_t* src_nrows, mirt_buf* const* dst, const uint32_t* dst_row0,
                       const uint32_t* dst_nrows, int n_ctx, size_t row_bytes) try {
    if (!live_group(g)) return fail(nullptr, MIRT_E_HANDLE, "mirt_exchange_rows: unknown group");
    const int n = (int)g->ctxs.size();
    mirt_ctx* const c0 = g->ctxs[0];
    // arguments first: nothing is flushed or queued on any device for a call that is going to be refused
    if (!src || !src_row0 || !src_nrows || !dst || !dst_row0 || !dst_nrows) return fail(c0, MIRT_E_ARG, "mirt_exchange_rows: null argument");
    if (n_ctx != n) return fail(c0, MIRT_E_ARG, "mirt_exchange_rows: %d entries for a group of %d contexts", n_ctx, n);
    if (!row_bytes || row_bytes % 4u) return fail(c0, MIRT_E_ARG, "mirt_exchange_rows: row_bytes %zu is not a positive multiple of 4", row_bytes);
    std::vector<pt::PostRange> rs((size_t)n), rd((size_t)n);
    for (int i = 0; i < n; ++i) {
        const struct { const char* what; mirt_buf* b; uint32_t rows; pt::PostRange* r; } side[2] = {{"source", src[i], src_nrows[i], &rs[(size_t)i]}, {"destination", dst[i], dst_nrows[i], &rd[(size_t)i]}};
        for (const auto& e : side) {
            *e.r = pt::PostRange{0, (uint64_t)e.rows * row_bytes, false};
            if (!e.b && !e.rows) continue;
            if (!live_has(e.b) || e.b->ctx != g->ctxs[(size_t)i]) return fail(c0, MIRT_E_HANDLE, "mirt_exchange_rows: %s %d is not a live buffer of the group's context %d", e.what, i, i);
            if ((uint64_t)e.b->bytes < e.r->bytes)
                return fail(c0, MIRT_E_RANGE, "mirt_exchange_rows: %s %d holds %zu bytes, %u rows of %zu bytes need %llu", e.what, i, e.b->bytes, e.rows, row_bytes, (unsigned long long)e.r->bytes);
            e.r->addr = (uint64_t)(uintptr_t)e.b->ptr;
            e.r->present = e.rows != 0u;
        }
    }
    std::vector<pt::RowCopy> plan;
    size_t at = 0;
    const pt::ExchangeVerdict v = pt::exchange_plan(src_row0, src_nrows, dst_row0, dst_nrows, (size_t)n, &plan, &at);
    if (v == pt::EXCHANGE_OWNERS_OVERLAP) return fail(c0, MIRT_E_ARG, "mirt_exchange_rows: source %zu owns rows that another source owns too", at);
    if (v == pt::EXCHANGE_ROW_UNOWNED) return fail(c0, MIRT_E_ARG, "mirt_exchange_rows: destination %zu wants a row that no source owns", at);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            if (pt::post_ranges_meet(rd[(size_t)i], rs[(size_t)j])) return fail(c0, MIRT_E_ARG, "mirt_exchange_rows: destination %d's bytes meet source %d's", i, j);
            if (j < i && pt::post_ranges_meet(rd[(size_t)i], rd[(size_t)j])) return fail(c0, MIRT_E_ARG, "mirt_exchange_rows: destination %d's bytes meet destination %d's", i, j);
        }
    for (int i = 0; i < n; ++i)   // (reported on context 0, like every refusal of this call: that is where a host looks)
        if (g->ctxs[(size_t)i]->capturing) return fail(c0, MIRT_E_ARG, "mirt_exchange_rows is not possible inside mirt_capture_begin/end (context %d is recording)", i);
    for (auto* c : g->ctxs) FLUSH_PENDING(c);
    // which destination reads which source across two streams (on one stream the order of the queue is the order)
    std::vector<uint8_t> reads((size_t)n * n, 0), src_read((size_t)n, 0), dst_waits((size_t)n, 0);
    for (const pt::RowCopy& c : plan)
        if (g->ctxs[c.src_ctx]->stream != g->ctxs[c.dst_ctx]->stream) { reads[(size_t)c.dst_ctx * n + c.src_ctx] = 1; src_read[c.src_ctx] = 1; dst_waits[c.dst_ctx] = 1; }
    EventSet es((size_t)n), ed((size_t)n);
    // 1. one event on every source's stream: the tile is written
    for (int s = 0; s < n; ++s) {
        if (!src_read[(size_t)s]) continue;
        mirt_ctx* c = g->ctxs[(size_t)s];
        HIPCHK(c0, hipSetDevice(c->device));
        HIPCHK(c0, hipEventCreateWithFlags(&es.ev[(size_t)s], hipEventDisableTiming));
        HIPCHK(c0, hipEventRecord(es.ev[(size_t)s], c->stream));
    }
    // 2. every destination's stream waits for the owners it reads, copies, and records that it has read them
    size_t k = 0;
    for (int d = 0; d < n; ++d) {
        if (k == plan.size() || plan[k].dst_ctx != (uint32_t)d) continue;   // the plan is ordered by destination
        mirt_ctx* c = g->ctxs[(size_t)d];
        HIPCHK(c0, hipSetDevice(c->device));
        for (int s = 0; s < n; ++s)
            if (reads[(size_t)d * n + s]) HIPCHK(c0, hipStreamWaitEvent(c->stream, es.ev[(size_t)s], 0));
        for (; k < plan.size() && plan[k].dst_ctx == (uint32_t)d; ++k) {
            const pt::RowCopy& cp = plan[k];
            mirt_ctx* sc = g->ctxs[cp.src_ctx];
            char* const to = (char*)dst[d]->ptr + (size_t)cp.dst_row * row_bytes;
            const char* const from = (const char*)src[cp.src_ctx]->ptr + (size_t)cp.src_row * row_bytes;
            const size_t bytes = (size_t)cp.nrows * row_bytes;
            if (sc->device == c->device) HIPCHK(c0, hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToDevice, c->stream));
            else HIPCHK(c0, hipMemcpyPeerAsync(to, c->device, from, sc->device, bytes, c->stream));
        }
        dst[d]->version++;
        if (dst_waits[(size_t)d]) {
            HIPCHK(c0, hipEventCreateWithFlags(&ed.ev[(size_t)d], hipEventDisableTiming));
            HIPCHK(c0, hipEventRecord(ed.ev[(size_t)d], c->stream));
        }
    }
    // 3. every source's stream waits for its readers: the next pass may overwrite the tile without a finish
    for (int s = 0; s < n; ++s) {
        if (!src_read[(size_t)s]) continue;
        mirt_ctx* c = g->ctxs[(size_t)s];
        HIPCHK(c0, hipSetDevice(c->device));
        for (int d = 0; d < n; ++d)
            if (reads[(size_t)d * n + s]) HIPCHK(c0, hipStreamWaitEvent(c->stream, ed.ev[(size_t)d], 0));
    }
    return MIRT_OK;
} MIRT_CATCH("mirt_exchange_rows", return MIRT_E_DEVICE)

int mirt_ctx_set_fusion(mirt_ctx* ctx, int level) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_ctx_set_fusion: unknown context");
    if (level != 0 && level != 2) return fail(ctx, MIRT_E_ARG, "mirt_ctx_set_fusion: level is 0 (every enqueue launches) or 2 (whole passes are fused)");
    FLUSH_PENDING(ctx);
    ctx->fusion = level;
    return MIRT_OK;
} MIRT_CATCH("mirt_ctx_set_fusion", return MIRT_E_DEVICE)

int mirt_ctx_fused_passes(mirt_ctx* ctx, uint64_t* count) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_ctx_fused_passes: unknown context");
    if (!count) return fail(ctx, MIRT_E_ARG, "mirt_ctx_fused_passes: null output");
    *count = ctx->fused_passes;
    return MIRT_OK;
} MIRT_CATCH("mirt_ctx_fused_passes", return MIRT_E_DEVICE)
int mirt_ctx_guided_passes(mirt_ctx* ctx, uint64_t* count) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_ctx_guided_passes: unknown context");
    if (!count) return fail(ctx, MIRT_E_ARG, "mirt_ctx_guided_passes: null output");
    *count = ctx->guided_passes;
    return MIRT_OK;
} MIRT_CATCH("mirt_ctx_guided_passes", return MIRT_E_DEVICE)

int mirt_ctx_set_frame_fusion(mirt_ctx* ctx, int on) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_ctx_set_frame_fusion: unknown context");
    FLUSH_PENDING(ctx);
    ctx->frame_fusion = on != 0;
    return MIRT_OK;
} MIRT_CATCH("mirt_ctx_set_frame_fusion", return MIRT_E_DEVICE)

int mirt_ctx_fused_frames(mirt_ctx* ctx, uint64_t* count) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_ctx_fused_frames: unknown context");
    if (!count) return fail(ctx, MIRT_E_ARG, "mirt_ctx_fused_frames: null output");
    *count = ctx->fused_frames;
    return MIRT_OK;
} MIRT_CATCH("mirt_ctx_fused_frames", return MIRT_E_DEVICE)

// A whole Assign04 / Assign07 frame in one launch (pt_kernels_frame.hip k_frame_fused).  Every check launch_kernel makes for initTrace and the trace
// kernels over the full image is made here, all of them before anything is prepared or launched.  aa > 1: mirt_render_frame_aa's frame, the same
// checks on the same descriptor (the caller has checked aa itself and that there is no ray buffer), then the FINE frame's arguments -- the camera block
// with aa times the columns and rows -- to the kernel that averages aa x aa of its samples into each of the descriptor's width x height pixels.
static int render_frame_impl(mirt_ctx* ctx, const mirt_frame_desc* d, uint32_t aa) {
    if (!d || d->struct_size != sizeof(mirt_frame_desc)) return fail(ctx, MIRT_E_ARG, "mirt_render_frame: descriptor size mismatch");
    if (d->assign != 4 && d->assign != 7) return fail(ctx, MIRT_E_ARG, "mirt_render_frame: assign %u (4 and 7 are frames of two launches; Assign01 is one launch already, Assign10 is mirt_render_pass)", d->assign);
    const bool mesh = d->t_pos != nullptr, mol = d->s_atoms != nullptr;
    if (!mesh && !mol) return fail(ctx, MIRT_E_ARG, "mirt_render_frame: no stage asked for (neither t_pos nor s_atoms)");
    if (d->assign == 4 && mol) return fail(ctx, MIRT_E_ARG, "mirt_render_frame: Assign04's molecule kernel is not built (its molecule mode is Assign07's)");
    if (!d->width || !d->height) return fail(ctx, MIRT_E_ARG, "mirt_render_frame: empty image");
    const uint32_t cols = f2u_host(d->cam[14]), rows = f2u_host(d->cam[15]);
    if (cols != d->width || rows != d->height) return fail(ctx, MIRT_E_ARG, "mirt_render_frame: camera says %ux%u, descriptor %ux%u", cols, rows, d->width, d->height);
    if (!d->pixel) return fail(ctx, MIRT_E_ARG, "mirt_render_frame: null pixel buffer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t npx = (uint64_t)cols * rows;
    int rc;
    if ((rc = need(ctx, "mirt_render_frame pixel", d->pixel, npx * 4))) return rc;
    if (d->rays && (rc = need(ctx, "mirt_render_frame rays", d->rays, npx * kRayBytes))) return rc;
    pt::FrameArgs A = {};
    memcpy(A.cam, d->cam, 64);
    A.assign = d->assign; A.mesh = mesh; A.mol = mol; A.gx = cols; A.gy = rows;
    if (d->assign == 4) {
        if (!d->t_normal || !d->t_mindex || !d->t_mcolor) return fail(ctx, MIRT_E_ARG, "mirt_render_frame: the Assign04 mesh needs t_normal, t_mindex and t_mcolor");
        if ((rc = frame_a04_mesh(ctx, "mirt_render_frame", d->t_size, d->t_pos, d->t_normal, d->t_mindex, d->t_mcolor, A))) return rc;
    } else {
        if (mol && !d->s_slab_size) return fail(ctx, MIRT_E_ARG, "mirt_render_frame: the molecule needs s_slab_size");
        if (mesh && (!d->t_normal || !d->t_slab_size)) return fail(ctx, MIRT_E_ARG, "mirt_render_frame: the Assign07 mesh needs t_normal and t_slab_size");
        if (mol && (rc = frame_a07_mol(ctx, "mirt_render_frame", d->bounds, d->n_slabs, d->s_slab_size, d->s_atoms, A))) return rc;
        if (mesh && (rc = frame_a07_mesh(ctx, "mirt_render_frame", d->bounds, d->n_slabs, d->t_slab_size, d->t_pos, d->t_normal, A))) return rc;
    }
    A.pixels = d->pixel->ptr;
    A.rays = d->rays ? d->rays->ptr : nullptr;
    if (aa > 1u) {
        A.gx = aa * cols; A.gy = aa * rows;   // at most 65535 each: exact as floats
        A.cam[14] = (float)A.gx; A.cam[15] = (float)A.gy;
        pt::launch_frame_aa(ctx->stream, A, aa, cols, rows);
    } else {
        pt::launch_frame_fused(ctx->stream, A);
    }
    HIPCHK(ctx, hipGetLastError());
    d->pixel->version++;
    if (d->rays) d->rays->version++;
    return MIRT_OK;
}

int mirt_render_frame(mirt_ctx* ctx, const mirt_frame_desc* d) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_render_frame: unknown context");
    FLUSH_PENDING(ctx);
    return render_frame_impl(ctx, d);
} MIRT_CATCH("mirt_render_frame", return MIRT_E_DEVICE)

int mirt_render_frame_aa(mirt_ctx* ctx, const mirt_frame_desc* d, uint32_t aa) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_render_frame_aa: unknown context");
    FLUSH_PENDING(ctx);
    if (aa < 1u || aa > 4u) return fail(ctx, MIRT_E_ARG, "mirt_render_frame_aa: aa %u (1 to 4 samples per axis)", aa);
    if (aa > 1u && d && d->struct_size == sizeof(mirt_frame_desc)) {
        if (d->rays) return fail(ctx, MIRT_E_ARG, "mirt_render_frame_aa: a ray buffer with aa %u (a pixel has no one ray)", aa);
        if ((uint64_t)aa * d->width > 65535u || (uint64_t)aa * d->height > 65535u)
            return fail(ctx, MIRT_E_ARG, "mirt_render_frame_aa: %ux%u at aa %u is a fine frame beyond 65535 samples per axis", d->width, d->height, aa);
    }
    return render_frame_impl(ctx, d, aa);
} MIRT_CATCH("mirt_render_frame_aa", return MIRT_E_DEVICE)

int mirt_ctx_set_exact_only(mirt_ctx* ctx, int on) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_ctx_set_exact_only: unknown context");
    FLUSH_PENDING(ctx);
    ctx->force_exact = on != 0;
    return MIRT_OK;
} MIRT_CATCH("mirt_ctx_set_exact_only", return MIRT_E_DEVICE)

int mirt_pass_deferred(mirt_ctx* ctx, uint64_t* samples) try {
    ENTRY_PROLOGUE(ctx, "mirt_pass_deferred");
    return count_deferred(ctx, "mirt_pass_deferred", ctx->pass_mask, samples);   // (resolving in the pass the exact kernel re-runs whole blocks of 256 samples)
} MIRT_CATCH("mirt_pass_deferred", return MIRT_E_DEVICE)

int mirt_ctx_set_profiling(mirt_ctx* ctx, int on) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_ctx_set_profiling: unknown context");
    FLUSH_PENDING(ctx);
    ctx->profiling = on != 0;
    ctx->pe_valid = false;
    return MIRT_OK;
} MIRT_CATCH("mirt_ctx_set_profiling", return MIRT_E_DEVICE)

int mirt_pass_timing(mirt_ctx* ctx, float* fused_ms, float* resolve_ms) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_pass_timing: unknown context");
    FLUSH_PENDING(ctx);
    if (!ctx->pe_valid) return fail(ctx, MIRT_E_ARG, "mirt_pass_timing: no profiled mirt_render_pass yet (mirt_ctx_set_profiling)");
    HIPCHK(ctx, hipEventSynchronize(ctx->pe[2]));
    float a = 0.f, b = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&a, ctx->pe[0], ctx->pe[1]));
    HIPCHK(ctx, hipEventElapsedTime(&b, ctx->pe[1], ctx->pe[2]));
    if (fused_ms) *fused_ms = a;
    if (resolve_ms) *resolve_ms = b;
    return MIRT_OK;
} MIRT_CATCH("mirt_pass_timing", return MIRT_E_DEVICE)

int mirt_seed_fill(mirt_ctx* ctx, mirt_buf* seeds, uint64_t first_ray, uint64_t count, uint32_t seed_base) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_seed_fill: unknown context");
    FLUSH_PENDING(ctx);
    int rc = need(ctx, "mirt_seed_fill", seeds, count * 4);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pt::launch_seedFill(ctx->stream, seeds->ptr, first_ray, count, seed_base);
    HIPCHK(ctx, hipGetLastError());
    seeds->version++;
    return MIRT_OK;
} MIRT_CATCH("mirt_seed_fill", return MIRT_E_DEVICE)

int mirt_zero(mirt_ctx* ctx, mirt_buf* buf) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_zero: unknown context");
    FLUSH_PENDING(ctx);
    int rc = need(ctx, "mirt_zero", buf, 0);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemsetAsync(buf->ptr, 0, buf->bytes, ctx->stream));
    buf->version++;
    return MIRT_OK;
} MIRT_CATCH("mirt_zero", return MIRT_E_DEVICE)

int mirt_debug_prepared(mirt_ctx* ctx, mirt_buf* positions, uint32_t count, void* out, size_t bytes, size_t* total) try {
    ENTRY_PROLOGUE(ctx, "mirt_debug_prepared");
    if (!live_has(positions) || positions->ctx != ctx) return fail(ctx, MIRT_E_HANDLE, "mirt_debug_prepared: unknown buffer");
    int rc = need(ctx, "mirt_debug_prepared positions", positions, (uint64_t)count * 48);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_prepared(ctx, positions, count))) return rc;
    const size_t have = pt::prepared_bytes(count);
    if (total) *total = have;
    if (out && bytes && positions->prep) {
        HIPCHK(ctx, hipMemcpyAsync(out, positions->prep, bytes < have ? bytes : have, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MIRT_OK;
} MIRT_CATCH("mirt_debug_prepared", return MIRT_E_DEVICE)

int mirt_debug_numerics(mirt_ctx* ctx, int op, mirt_buf* a, mirt_buf* b, mirt_buf* out, size_t n) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_debug_numerics: unknown context");
    FLUSH_PENDING(ctx);
    int rc;
    if (!((op >= 0 && op <= 14) || (op >= 20 && op <= 28))) return fail(ctx, MIRT_E_ARG, "mirt_debug_numerics: op %d outside 0..14, 20..28", op);
    const bool vec = op >= 20 && op != 25;
    const uint64_t in_w = vec ? 3 : 1, out_w = (op == 21 || op == 24) ? 3 : op == 27 ? 4 : 1;
    const bool two = op == 0 || (op >= 6 && op <= 12) || op == 20 || op == 21 || op == 23 || op == 25 || op == 28;
    if ((rc = need(ctx, "mirt_debug_numerics a", a, (uint64_t)n * 4 * in_w))) return rc;
    if (two && !b) return fail(ctx, MIRT_E_ARG, "mirt_debug_numerics: op %d needs two inputs", op);
    if (b && (rc = need(ctx, "mirt_debug_numerics b", b, (uint64_t)n * 4 * (two ? in_w : 1)))) return rc;
    if ((rc = need(ctx, "mirt_debug_numerics out", out, (uint64_t)n * 4 * out_w))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pt::launch_numerics(ctx->stream, op, a->ptr, b ? b->ptr : nullptr, out->ptr, n);
    HIPCHK(ctx, hipGetLastError());
    return MIRT_OK;
} MIRT_CATCH("mirt_debug_numerics", return MIRT_E_DEVICE)

static int new_owned(mirt_ctx* ctx, size_t bytes, mirt_buf** out) {
    return mirt_buf_create(ctx, bytes ? bytes : 16, MIRT_MEM_READ_WRITE, out);
}

int mirt_grid_build(mirt_ctx* ctx, const mirt_grid_build_desc* d, mirt_buf** cell_offsets, mirt_buf** order, uint32_t* total) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_grid_build: unknown context");
    FLUSH_PENDING(ctx);
    if (!d || d->struct_size != sizeof(mirt_grid_build_desc) || !cell_offsets || !order || !total)
        return fail(ctx, MIRT_E_ARG, "mirt_grid_build: null argument or descriptor size mismatch");
    *cell_offsets = *order = nullptr;
    *total = 0;
    if (d->kind > 1) return fail(ctx, MIRT_E_ARG, "mirt_grid_build: kind is 0 (spheres) or 1 (triangles)");
    if (d->n_slabs == 0 || d->n_slabs > 1024) return fail(ctx, MIRT_E_ARG, "mirt_grid_build: n_slabs %u outside 1..1024", d->n_slabs);
    int rc;
    if (d->count && (rc = need(ctx, "mirt_grid_build prims", d->prims_f64, (uint64_t)d->count * (d->kind ? 72 : 32)))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t cells = (uint64_t)d->n_slabs * d->n_slabs * d->n_slabs;
    if ((rc = new_owned(ctx, (cells + 1) * 4, cell_offsets))) return rc;
    uint32_t* ord = nullptr;
    uint64_t slots = 0;
    hipError_t e = pt::grid_build(ctx->stream, (int)d->kind, d->count ? (const double*)d->prims_f64->ptr : nullptr, d->count, d->bounds, d->n_slabs,
                                  (uint32_t*)(*cell_offsets)->ptr, &ord, total, &slots);
    if (e != hipSuccess || slots > pt::kMaxGridSlots) {
        mirt_buf_release(*cell_offsets);
        *cell_offsets = nullptr;
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(ctx, MIRT_E_DEVICE, "mirt_grid_build: %s", hipGetErrorString(e)); }
        return fail(ctx, MIRT_E_RANGE, "mirt_grid_build: the grid would hold %llu (cell, primitive) slots; at most %llu are supported -- use fewer slabs",
                    (unsigned long long)slots, (unsigned long long)pt::kMaxGridSlots);
    }
    // adopt the order array as an owned buffer
    mirt_buf* ob = new mirt_buf();
    ob->ctx = ctx; ob->bytes = *total ? (size_t)*total * 4 : 16; ob->owned = true; ob->flags = MIRT_MEM_READ_WRITE; ob->uid = g_next_uid++;
    if (ord) ob->ptr = ord;
    else if (hipMalloc(&ob->ptr, 16) != hipSuccess) { delete ob; return fail(ctx, MIRT_E_DEVICE, "mirt_grid_build: hipMalloc failed"); }
    live_add(ob, H_BUF);
    ctx->bufs.insert(ob);
    *order = ob;
    (*cell_offsets)->version++;
    return MIRT_OK;
} MIRT_CATCH("mirt_grid_build", return MIRT_E_DEVICE)

int mirt_grid_gather_triangles(mirt_ctx* ctx, mirt_buf* order, uint32_t total, mirt_buf* pos_f64, mirt_buf* nor_f64, uint32_t nsteps,
                               const int32_t* ops, const double* vecs, float pad_w, mirt_buf** pos_out, mirt_buf** nor_out) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_grid_gather_triangles: unknown context");
    FLUSH_PENDING(ctx);
    if (!pos_out || nsteps > 4 || (nsteps && (!ops || !vecs))) return fail(ctx, MIRT_E_ARG, "mirt_grid_gather_triangles: bad argument");
    for (uint32_t i = 0; i < nsteps; ++i) if (ops[i] < 0 || ops[i] > 2) return fail(ctx, MIRT_E_ARG, "mirt_grid_gather_triangles: op %d", ops[i]);
    int rc;
    if ((rc = need(ctx, "gather order", order, (uint64_t)total * 4))) return rc;
    if ((rc = need(ctx, "gather positions", pos_f64, 0))) return rc;
    if (nor_f64 && nor_out && (rc = need(ctx, "gather normals", nor_f64, 0))) return rc;
    if (pos_f64->bytes % 72) return fail(ctx, MIRT_E_ARG, "mirt_grid_gather_triangles: positions are 9 doubles per triangle");
    // every index in `order` must address a triangle of the inputs: order comes from mirt_grid_build over `count` primitives;
    // a foreign order array is checked on the host
    if (total) {
        std::vector<uint32_t> h(total);
        HIPCHK(ctx, hipMemcpyAsync(h.data(), order->ptr, (size_t)total * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        const uint64_t ntri = pos_f64->bytes / 72;
        for (uint32_t v : h) if (v >= ntri) return fail(ctx, MIRT_E_DATA, "mirt_grid_gather_triangles: order refers to triangle %u of %llu", v, (unsigned long long)ntri);
        if (nor_f64 && nor_out && nor_f64->bytes < ntri * 72) return fail(ctx, MIRT_E_RANGE, "mirt_grid_gather_triangles: normals shorter than positions");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = new_owned(ctx, (size_t)total * 48, pos_out))) return rc;
    const bool want_n = nor_f64 && nor_out;
    if (nor_out) *nor_out = nullptr;
    if (want_n && (rc = new_owned(ctx, (size_t)total * 48, nor_out))) return rc;
    pt::launch_gatherTriangles(ctx->stream, (const uint32_t*)order->ptr, total, (const double*)pos_f64->ptr, want_n ? (const double*)nor_f64->ptr : nullptr,
                               (int)nsteps, (const int*)ops, vecs, pad_w, (*pos_out)->ptr, want_n ? (*nor_out)->ptr : nullptr);
    HIPCHK(ctx, hipGetLastError());
    (*pos_out)->version++;
    return MIRT_OK;
} MIRT_CATCH("mirt_grid_gather_triangles", return MIRT_E_DEVICE)

int mirt_mesh_ingest(mirt_ctx* ctx, const mirt_mesh_ingest_desc* d, mirt_buf* pos9_out, mirt_buf* nor9_out, mirt_buf* bounds6) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_mesh_ingest: unknown context");
    FLUSH_PENDING(ctx);
    if (!d || d->struct_size != sizeof(mirt_mesh_ingest_desc)) return fail(ctx, MIRT_E_ARG, "mirt_mesh_ingest: null descriptor or size mismatch");
    NOT_WHILE_CAPTURING(ctx, "mirt_mesh_ingest");
    if (d->n_corners % 3u) return fail(ctx, MIRT_E_ARG, "mirt_mesh_ingest: %u corners is not a whole number of triangles", d->n_corners);
    int rc;
    if ((rc = need(ctx, "mirt_mesh_ingest positions", d->positions_f64, (uint64_t)d->n_vertices * 24))) return rc;
    if ((rc = need(ctx, "mirt_mesh_ingest normals", d->normals_f64, (uint64_t)d->n_vertices * 24))) return rc;
    if (d->indices_u32 && (rc = need(ctx, "mirt_mesh_ingest indices", d->indices_u32, (uint64_t)d->n_corners * 4))) return rc;
    if (!d->indices_u32 && d->n_corners > d->n_vertices) return fail(ctx, MIRT_E_RANGE, "mirt_mesh_ingest: %u corners of an un-indexed mesh with %u vertices", d->n_corners, d->n_vertices);
    const uint64_t end = ((uint64_t)d->first_corner + d->n_corners) * 24;
    if ((rc = need(ctx, "mirt_mesh_ingest positions out", pos9_out, end))) return rc;
    if ((rc = need(ctx, "mirt_mesh_ingest normals out", nor9_out, end))) return rc;
    if ((rc = need(ctx, "mirt_mesh_ingest bounds", bounds6, 24))) return rc;
    if ((rc = ensure_scratch(ctx, 32))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemsetAsync(ctx->scratch, 0, 32, ctx->stream));
    pt::launch_meshIngest(ctx->stream, (const double*)d->positions_f64->ptr, (const double*)d->normals_f64->ptr,
                          d->indices_u32 ? (const uint32_t*)d->indices_u32->ptr : nullptr, d->n_vertices, d->n_corners, d->model, d->normal_mat,
                          (double*)pos9_out->ptr + 3u * (size_t)d->first_corner, (double*)nor9_out->ptr + 3u * (size_t)d->first_corner,
                          (float*)bounds6->ptr, (uint32_t*)ctx->scratch);
    uint32_t flag = 0;
    HIPCHK(ctx, hipMemcpyAsync(&flag, (const char*)ctx->scratch + 24, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    pos9_out->version++; nor9_out->version++; bounds6->version++;
    if (flag) return fail(ctx, MIRT_E_DATA, "mirt_mesh_ingest: an index refers past the %u vertices of the mesh", d->n_vertices);
    return MIRT_OK;
} MIRT_CATCH("mirt_mesh_ingest", return MIRT_E_DEVICE)

static int check_order(mirt_ctx* ctx, mirt_buf* order, uint32_t total, uint64_t n_in) {
    if (!total) return MIRT_OK;
    std::vector<uint32_t> h(total);
    HIPCHK(ctx, hipMemcpyAsync(h.data(), order->ptr, (size_t)total * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t v : h) if (v >= n_in) return fail(ctx, MIRT_E_DATA, "order refers to element %u of %llu", v, (unsigned long long)n_in);
    return MIRT_OK;
}

int mirt_grid_gather_spheres(mirt_ctx* ctx, mirt_buf* order, uint32_t total, mirt_buf* sph_f64, mirt_buf** out) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_grid_gather_spheres: unknown context");
    FLUSH_PENDING(ctx);
    if (!out) return fail(ctx, MIRT_E_ARG, "mirt_grid_gather_spheres: null out");
    int rc;
    if ((rc = need(ctx, "gather order", order, (uint64_t)total * 4))) return rc;
    if ((rc = need(ctx, "gather spheres", sph_f64, 0))) return rc;
    if ((rc = check_order(ctx, order, total, sph_f64->bytes / 32))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = new_owned(ctx, (size_t)total * 16, out))) return rc;
    pt::launch_gatherSpheres(ctx->stream, (const uint32_t*)order->ptr, total, (const double*)sph_f64->ptr, (*out)->ptr);
    HIPCHK(ctx, hipGetLastError());
    (*out)->version++;
    return MIRT_OK;
} MIRT_CATCH("mirt_grid_gather_spheres", return MIRT_E_DEVICE)

int mirt_grid_gather_u32(mirt_ctx* ctx, mirt_buf* order, uint32_t total, mirt_buf* in_u32, mirt_buf** out) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_grid_gather_u32: unknown context");
    FLUSH_PENDING(ctx);
    if (!out) return fail(ctx, MIRT_E_ARG, "mirt_grid_gather_u32: null out");
    int rc;
    if ((rc = need(ctx, "gather order", order, (uint64_t)total * 4))) return rc;
    if ((rc = need(ctx, "gather input", in_u32, 0))) return rc;
    if ((rc = check_order(ctx, order, total, in_u32->bytes / 4))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = new_owned(ctx, (size_t)total * 4, out))) return rc;
    pt::launch_gatherU32(ctx->stream, (const uint32_t*)order->ptr, total, (const uint32_t*)in_u32->ptr, (uint32_t*)(*out)->ptr);
    HIPCHK(ctx, hipGetLastError());
    (*out)->version++;
    return MIRT_OK;
} MIRT_CATCH("mirt_grid_gather_u32", return MIRT_E_DEVICE)

int mirt_debug_divcheck(mirt_ctx* ctx, int mode, uint64_t seed, uint64_t count, mirt_buf* out16) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_debug_divcheck: unknown context");
    FLUSH_PENDING(ctx);
    int rc = need(ctx, "mirt_debug_divcheck out", out16, 16 * 8);
    if (rc) return rc;
    if (mode < 0 || mode > 6) return fail(ctx, MIRT_E_ARG, "mirt_debug_divcheck: mode is 0..6");
    if (mode == 4 && (seed > (1u << 23) || count > (1u << 23) - seed)) return fail(ctx, MIRT_E_ARG, "mirt_debug_divcheck: mode 4 walks denominators [seed, seed+count) within 2^23 mantissas");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemsetAsync(out16->ptr, 0, 16 * 8, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync((char*)out16->ptr + 80, 0xFF, 8, ctx->stream));   // out[10]: running minimum
    pt::launch_divCheck(ctx->stream, mode, seed, count, out16->ptr);
    HIPCHK(ctx, hipGetLastError());
    return MIRT_OK;
} MIRT_CATCH("mirt_debug_divcheck", return MIRT_E_DEVICE)

int mirt_capture_begin(mirt_ctx* ctx) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_capture_begin: unknown context");
    FLUSH_PENDING(ctx);
    if (ctx->capturing) return fail(ctx, MIRT_E_ARG, "mirt_capture_begin: already recording");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed));
    ctx->capturing = true;
    ctx->cap_pins.clear();
    ctx->cap_scratch = ctx->cap_defer = false;
    return MIRT_OK;
} MIRT_CATCH("mirt_capture_begin", return MIRT_E_DEVICE)

int mirt_capture_end(mirt_ctx* ctx, mirt_graph** out) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_capture_end: unknown context");
    if (!out) return fail(ctx, MIRT_E_ARG, "mirt_capture_end: null output");
    if (!ctx->capturing) return fail(ctx, MIRT_E_ARG, "mirt_capture_end: not recording");
    ctx->capturing = false;
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(ctx->stream, &g);
    if (e != hipSuccess || !g) {
        (void)hipGetLastError();
        return fail(ctx, MIRT_E_DEVICE, "mirt_capture_end: the recording was invalidated (%s)", hipGetErrorString(e));
    }
    hipGraphExec_t x = nullptr;
    e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(g);
        return fail(ctx, MIRT_E_DEVICE, "mirt_capture_end: hipGraphInstantiate: %s", hipGetErrorString(e));
    }
    mirt_graph* mg = new mirt_graph;
    mg->ctx = ctx; mg->graph = g; mg->exec = x;
    mg->pins.swap(ctx->cap_pins);
    mg->scratch_gen = ctx->cap_scratch ? ctx->scratch_gen : 0;
    mg->defer_gen = ctx->cap_defer ? ctx->defer_gen : 0;
    live_add(mg, H_GRAPH);
    ctx->graphs.insert(mg);
    *out = mg;
    return MIRT_OK;
} MIRT_CATCH("mirt_capture_end", return MIRT_E_DEVICE)

int mirt_graph_launch(mirt_ctx* ctx, mirt_graph* graph) try {
    if (!live_has(ctx)) return fail(nullptr, MIRT_E_HANDLE, "mirt_graph_launch: unknown context");
    FLUSH_PENDING(ctx);
    if (!live_has(graph) || graph->ctx != ctx) return fail(ctx, MIRT_E_HANDLE, "mirt_graph_launch: unknown graph");
    NOT_WHILE_CAPTURING(ctx, "mirt_graph_launch");
    // the recording holds raw device pointers: refuse to replay once any of them has been freed, replaced or (for validated /
    // prepared geometry) rewritten since -- record the sequence again
    for (const auto& p : graph->pins) {
        if (!live_has(p.buf) || p.buf->uid != p.uid)
            return fail(ctx, MIRT_E_HANDLE, "mirt_graph_launch: a buffer the recording uses has been released; record the sequence again");
        if (p.content && (p.buf->version != p.version || p.buf->prep_gen != p.prep_gen))
            return fail(ctx, MIRT_E_HANDLE, "mirt_graph_launch: geometry the recording was validated against has been rewritten; record the sequence again");
    }
    if ((graph->scratch_gen && graph->scratch_gen != ctx->scratch_gen) || (graph->defer_gen && graph->defer_gen != ctx->defer_gen))
        return fail(ctx, MIRT_E_HANDLE, "mirt_graph_launch: the context's scratch memory was reallocated after the recording; record the sequence again");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipGraphLaunch(graph->exec, ctx->stream));
    return MIRT_OK;
} MIRT_CATCH("mirt_graph_launch", return MIRT_E_DEVICE)

int mirt_graph_release(mirt_graph* graph) try {
    if (!live_has(graph)) return fail(nullptr, MIRT_E_HANDLE, "mirt_graph_release: unknown graph");
    free_graph(graph, live_has(graph->ctx));
    return MIRT_OK;
} MIRT_CATCH("mirt_graph_release", return MIRT_E_DEVICE)

int mirt_timer_start(mirt_ctx* ctx) try {
    ENTRY_PROLOGUE(ctx, "mirt_timer_start");
    HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    return MIRT_OK;
} MIRT_CATCH("mirt_timer_start", return MIRT_E_DEVICE)

int mirt_timer_stop_ms(mirt_ctx* ctx, float* ms) try {
    ENTRY_PROLOGUE(ctx, "mirt_timer_stop_ms");
    if (!ms) return fail(ctx, MIRT_E_ARG, "mirt_timer_stop_ms: null output");
    HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
    HIPCHK(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return MIRT_OK;
} MIRT_CATCH("mirt_timer_stop_ms", return MIRT_E_DEVICE)

}  // extern "C"

#if PT_COUNT
// profiling builds only (-DPT_COUNT=1, profiles/trip_counts.py): the fused pass's wave-level trip counters (pt_trace.hpp PtCounter); not in include/mirt.h
namespace pt { int debug_counters(unsigned long long* out, int reset); }
extern "C" MIRT_API int mirt_debug_counters(unsigned long long* out32, int reset) { return pt::debug_counters(out32, reset); }
#endif
