// mirt_napi.cc -- N-API addon (raw node_api.h, N-API v3+; Node 12 has no napi.h wrapper here).
//
// A thin, flat binding of include/mirt.h for the JavaScript host: every export is one
// mirt_* call.  Handles travel as napi_external values.  Errors become JS exceptions whose
// `.code` is the mirt_status name and whose message is mirt_last_error().  The WebCL-shaped
// object model the reference host drives (webcl.getPlatforms() ... kernel.setArg ...) is
// built on top of these in host/webcl.js, in JavaScript.
#include <node_api.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/mirt.h"

namespace {

const char* status_name(int rc) {
    switch (rc) {
        case MIRT_E_ARG: return "MIRT_E_ARG";
        case MIRT_E_HANDLE: return "MIRT_E_HANDLE";
        case MIRT_E_NAME: return "MIRT_E_NAME";
        case MIRT_E_UNSET: return "MIRT_E_UNSET";
        case MIRT_E_RANGE: return "MIRT_E_RANGE";
        case MIRT_E_DEVICE: return "MIRT_E_DEVICE";
        case MIRT_E_NODEVICE: return "MIRT_E_NODEVICE";
        case MIRT_E_DATA: return "MIRT_E_DATA";
        default: return "MIRT_E_UNKNOWN";
    }
}

napi_value throw_mirt(napi_env env, int rc, mirt_ctx* ctx) {
    napi_throw_error(env, status_name(rc), mirt_last_error(ctx));
    return nullptr;
}
napi_value throw_type(napi_env env, const char* msg) {
    napi_throw_type_error(env, "MIRT_E_ARG", msg);
    return nullptr;
}

#define ARGS(n)                                                         \
    size_t argc = (n);                                                  \
    napi_value argv[(n) > 0 ? (n) : 1];                                 \
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok) return throw_type(env, "bad call"); \
    if (argc < (size_t)(n)) return throw_type(env, "too few arguments")

bool get_ext(napi_env env, napi_value v, void** out) {
    napi_valuetype t;
    if (napi_typeof(env, v, &t) != napi_ok || t != napi_external) return false;
    return napi_get_value_external(env, v, out) == napi_ok;
}
bool get_u32(napi_env env, napi_value v, uint32_t* out) { return napi_get_value_uint32(env, v, out) == napi_ok; }
bool get_f64(napi_env env, napi_value v, double* out) { return napi_get_value_double(env, v, out) == napi_ok; }
bool get_bytes(napi_env env, napi_value v, void** data, size_t* nbytes) {
    bool is_ta = false;
    if (napi_is_typedarray(env, v, &is_ta) != napi_ok) return false;
    if (is_ta) {
        napi_typedarray_type t;
        size_t len;
        napi_value ab;
        size_t off;
        if (napi_get_typedarray_info(env, v, &t, &len, data, &ab, &off) != napi_ok) return false;
        size_t es = 1;
        switch (t) {
            case napi_int16_array: case napi_uint16_array: es = 2; break;
            case napi_int32_array: case napi_uint32_array: case napi_float32_array: es = 4; break;
            case napi_float64_array: es = 8; break;
            default: es = 1; break;
        }
        *nbytes = len * es;
        return true;
    }
    bool is_ab = false;
    if (napi_is_arraybuffer(env, v, &is_ab) == napi_ok && is_ab) return napi_get_arraybuffer_info(env, v, data, nbytes) == napi_ok;
    return false;
}
napi_value mk_ext(napi_env env, void* p) { napi_value v; napi_create_external(env, p, nullptr, nullptr, &v); return v; }
napi_value mk_num(napi_env env, double d) { napi_value v; napi_create_double(env, d, &v); return v; }
napi_value undef(napi_env env) { napi_value v; napi_get_undefined(env, &v); return v; }

bool prop(napi_env env, napi_value obj, const char* name, napi_value* out) {
    bool has = false;
    if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return false;
    if (napi_get_named_property(env, obj, name, out) != napi_ok) return false;
    napi_valuetype t;
    napi_typeof(env, *out, &t);
    return t != napi_undefined && t != napi_null;
}
bool prop_u32(napi_env env, napi_value obj, const char* name, uint32_t* out) { napi_value v; return prop(env, obj, name, &v) && get_u32(env, v, out); }
bool prop_f32(napi_env env, napi_value obj, const char* name, float* out) { napi_value v; double d; if (!prop(env, obj, name, &v) || !get_f64(env, v, &d)) return false; *out = (float)d; return true; }
bool prop_floats(napi_env env, napi_value obj, const char* name, float* dst, size_t n) {
    napi_value v; void* data; size_t nb;
    if (!prop(env, obj, name, &v) || !get_bytes(env, v, &data, &nb) || nb < n * 4) return false;
    memcpy(dst, data, n * 4);
    return true;
}
mirt_buf* prop_buf(napi_env env, napi_value obj, const char* name) { napi_value v; void* p = nullptr; if (prop(env, obj, name, &v) && get_ext(env, v, &p)) return (mirt_buf*)p; return nullptr; }

// ---- exports --------------------------------------------------------------------------
napi_value DeviceCount(napi_env env, napi_callback_info) { return mk_num(env, mirt_device_count()); }

napi_value DeviceName(napi_env env, napi_callback_info info) {
    ARGS(1);
    uint32_t d;
    if (!get_u32(env, argv[0], &d)) return throw_type(env, "deviceName(index)");
    char buf[256];
    int rc = mirt_device_name((int)d, buf, sizeof buf);
    if (rc) return throw_mirt(env, rc, nullptr);
    napi_value s;
    napi_create_string_utf8(env, buf, NAPI_AUTO_LENGTH, &s);
    return s;
}

napi_value Version(napi_env env, napi_callback_info) { napi_value s; napi_create_string_utf8(env, mirt_version(), NAPI_AUTO_LENGTH, &s); return s; }

napi_value CtxCreate(napi_env env, napi_callback_info info) {
    ARGS(1);
    uint32_t d;
    if (!get_u32(env, argv[0], &d)) return throw_type(env, "ctxCreate(device)");
    mirt_ctx* c = nullptr;
    int rc = mirt_ctx_create((int)d, &c);
    if (rc) return throw_mirt(env, rc, nullptr);
    return mk_ext(env, c);
}
napi_value CtxDestroy(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "ctxDestroy(ctx)");
    int rc = mirt_ctx_destroy((mirt_ctx*)c);
    if (rc) return throw_mirt(env, rc, nullptr);
    return undef(env);
}
napi_value Finish(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "finish(ctx)");
    int rc = mirt_finish((mirt_ctx*)c);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
napi_value CtxSetFusion(napi_env env, napi_callback_info info) {
    ARGS(2);
    void* c; uint32_t level;
    if (!get_ext(env, argv[0], &c) || !get_u32(env, argv[1], &level)) return throw_type(env, "ctxSetFusion(ctx, level)");
    int rc = mirt_ctx_set_fusion((mirt_ctx*)c, (int)level);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
napi_value CtxFusedPasses(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "ctxFusedPasses(ctx)");
    uint64_t n = 0;
    int rc = mirt_ctx_fused_passes((mirt_ctx*)c, &n);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return mk_num(env, (double)n);
}
napi_value CtxGuidedPasses(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "ctxGuidedPasses(ctx)");
    uint64_t n = 0;
    int rc = mirt_ctx_guided_passes((mirt_ctx*)c, &n);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return mk_num(env, (double)n);
}
napi_value BufCreate(napi_env env, napi_callback_info info) {
    ARGS(3);
    void* c; double bytes; uint32_t flags;
    if (!get_ext(env, argv[0], &c) || !get_f64(env, argv[1], &bytes) || !get_u32(env, argv[2], &flags)) return throw_type(env, "bufCreate(ctx, bytes, flags)");
    mirt_buf* b = nullptr;
    int rc = mirt_buf_create((mirt_ctx*)c, bytes < 0 ? 0 : (size_t)bytes, flags, &b);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return mk_ext(env, b);
}
napi_value BufRelease(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* b;
    if (!get_ext(env, argv[0], &b)) return throw_type(env, "bufRelease(buf)");
    int rc = mirt_buf_release((mirt_buf*)b);
    if (rc) return throw_mirt(env, rc, nullptr);
    return undef(env);
}
napi_value BufSize(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* b;
    if (!get_ext(env, argv[0], &b)) return throw_type(env, "bufSize(buf)");
    return mk_num(env, (double)mirt_buf_size((mirt_buf*)b));
}
napi_value BufRW(napi_env env, napi_callback_info info, bool write) {
    ARGS(4);
    void* b; double off, n; void* data; size_t nb;
    if (!get_ext(env, argv[0], &b) || !get_f64(env, argv[1], &off) || !get_f64(env, argv[2], &n) || !get_bytes(env, argv[3], &data, &nb))
        return throw_type(env, "buf{Write,Read}(buf, offset, nbytes, typedArray)");
    if (off < 0 || n < 0 || (size_t)n > nb) return throw_type(env, "nbytes exceeds the typed array");
    int rc = write ? mirt_buf_write((mirt_buf*)b, (size_t)off, (size_t)n, data, 0) : mirt_buf_read((mirt_buf*)b, (size_t)off, (size_t)n, data, 1);
    if (rc) return throw_mirt(env, rc, nullptr);
    return undef(env);
}
napi_value BufWrite(napi_env env, napi_callback_info info) { return BufRW(env, info, true); }
napi_value BufRead(napi_env env, napi_callback_info info) { return BufRW(env, info, false); }

napi_value ProgramCheck(napi_env env, napi_callback_info info) {
    ARGS(2);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "programCheck(ctx, source)");
    size_t len = 0;
    if (napi_get_value_string_utf8(env, argv[1], nullptr, 0, &len) != napi_ok) return throw_type(env, "programCheck: source must be a string");
    std::string src(len + 1, '\0');
    napi_get_value_string_utf8(env, argv[1], &src[0], len + 1, &len);
    char missing[2048];
    int n = mirt_program_check((mirt_ctx*)c, src.c_str(), missing, sizeof missing);
    if (n < 0) return throw_mirt(env, n, (mirt_ctx*)c);
    napi_value o, s;
    napi_create_object(env, &o);
    napi_set_named_property(env, o, "missing", mk_num(env, n));
    napi_create_string_utf8(env, missing, NAPI_AUTO_LENGTH, &s);
    napi_set_named_property(env, o, "log", s);
    return o;
}

napi_value ProgramDialect(napi_env env, napi_callback_info info) {
    ARGS(1);
    size_t len = 0;
    if (napi_get_value_string_utf8(env, argv[0], nullptr, 0, &len) != napi_ok) return throw_type(env, "programDialect(source)");
    std::string src(len + 1, '\0');
    napi_get_value_string_utf8(env, argv[0], &src[0], len + 1, &len);
    return mk_num(env, mirt_program_dialect(src.c_str()));
}

napi_value KernelGet(napi_env env, napi_callback_info info) {
    ARGS(2);
    void* c; char name[128]; size_t len;
    if (!get_ext(env, argv[0], &c) || napi_get_value_string_utf8(env, argv[1], name, sizeof name, &len) != napi_ok) return throw_type(env, "kernelGet(ctx, name)");
    mirt_kernel* k = nullptr;
    int rc = mirt_kernel_get((mirt_ctx*)c, name, &k);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return mk_ext(env, k);
}
napi_value KernelRelease(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* k;
    if (!get_ext(env, argv[0], &k)) return throw_type(env, "kernelRelease(kernel)");
    int rc = mirt_kernel_release((mirt_kernel*)k);
    if (rc) return throw_mirt(env, rc, nullptr);
    return undef(env);
}
napi_value KernelNumArgs(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* k;
    if (!get_ext(env, argv[0], &k)) return throw_type(env, "kernelNumArgs(kernel)");
    return mk_num(env, mirt_kernel_num_args((mirt_kernel*)k));
}
napi_value KernelPreferredMultiple(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* k;
    if (!get_ext(env, argv[0], &k)) return throw_type(env, "kernelPreferredMultiple(kernel)");
    return mk_num(env, mirt_kernel_preferred_multiple((mirt_kernel*)k));
}
// kernelSetArg(kernel, index, typedArray | bufferHandle)
napi_value KernelSetArg(napi_env env, napi_callback_info info) {
    ARGS(3);
    void* k; uint32_t idx;
    if (!get_ext(env, argv[0], &k) || !get_u32(env, argv[1], &idx)) return throw_type(env, "kernelSetArg(kernel, index, value)");
    void* p; size_t nb; int rc;
    if (get_ext(env, argv[2], &p)) rc = mirt_kernel_set_arg_buf((mirt_kernel*)k, idx, (mirt_buf*)p);
    else if (get_bytes(env, argv[2], &p, &nb)) rc = mirt_kernel_set_arg((mirt_kernel*)k, idx, nb, p);
    else return throw_type(env, "kernelSetArg: value must be a typed array or a buffer");
    if (rc) return throw_mirt(env, rc, nullptr);
    return undef(env);
}
bool get_sizes(napi_env env, napi_value arr, std::vector<size_t>* out) {
    bool is_arr = false;
    if (napi_is_array(env, arr, &is_arr) != napi_ok || !is_arr) return false;
    uint32_t n;
    napi_get_array_length(env, arr, &n);
    for (uint32_t i = 0; i < n; ++i) {
        napi_value e; double d;
        napi_get_element(env, arr, i, &e);
        if (!get_f64(env, e, &d) || d < 0) return false;
        out->push_back((size_t)d);
    }
    return true;
}
napi_value Enqueue(napi_env env, napi_callback_info info) {
    ARGS(5);
    void *c, *k; uint32_t dim;
    std::vector<size_t> g, l;
    if (!get_ext(env, argv[0], &c) || !get_ext(env, argv[1], &k) || !get_u32(env, argv[2], &dim) || !get_sizes(env, argv[3], &g))
        return throw_type(env, "enqueue(ctx, kernel, dim, globalWS[], localWS[]|null)");
    bool has_local = get_sizes(env, argv[4], &l);
    if (g.size() < dim || (has_local && l.size() < dim)) return throw_type(env, "enqueue: work-size arrays shorter than dim");
    int rc = mirt_enqueue((mirt_ctx*)c, (mirt_kernel*)k, dim, g.data(), has_local ? l.data() : nullptr);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}

bool read_grid(napi_env env, napi_value o, mirt_grid* g) {
    memset(g, 0, sizeof *g);
    g->prims = prop_buf(env, o, "prims");
    g->normals = prop_buf(env, o, "normals");
    g->matid = prop_buf(env, o, "matid");
    g->cell_offsets = prop_buf(env, o, "cellOffsets");
    prop_u32(env, o, "meshMatId", &g->mesh_matid);
    return prop_floats(env, o, "bounds", g->bounds, 8) && prop_u32(env, o, "nSlabs", &g->n_slabs);
}
// renderPass(ctx, {width,height,raysPerPixel,row0,nrows,bounces,passIndex,cam,sceneBounds,focalLength,lensRad,
//                  spheres?,triangles?,meshes[],lights[{shadow,scene,light}],material,seeds,acu,pixel?,radiance?})
// desc.nPasses: that many passes in one call (mirt_render_passes; desc.firstPass -> MIRT_PASSES_FRESH, desc.everyPass -> MIRT_PASSES_EVERY_FRAME: pixel /
// radiance hold nPasses frames; webcl.js checks the count's range and the frame buffers' sizes)
// renderGuides(ctx, desc, normalHits, albedoDepth): the same descriptor (seeds, acu, pixel, radiance, lights are not needed), two float4-per-pixel
// buffers of the tile, either may be null (mirt_render_guides)
// renderFirstPassGuided(ctx, desc, normalHits, albedoDepth): the frame's first pass of the descriptor and its guides in one call
// (mirt_render_first_pass_guided)
// renderPassesGuided(ctx, desc, normalHits, albedoDepth): desc.nPasses passes (desc.firstPass, desc.everyPass as for renderPass) and the frame's
// guides in one call (mirt_render_passes_guided)
// renderAo(ctx, desc, aoDesc, aoOut): ambient occlusion of the first hit of the same descriptor (seeds are read, not written; material, lights,
// acu, pixel, radiance are not needed), aoDesc = {samples, radius, bias} -- a number left out is the header's default, radius +Infinity --, aoOut
// uint32 {open, cast} per pixel of the tile (mirt_render_ao).  aoDeferred(ctx) -> the pixels the last renderAo re-ran in the exact kernel.
// The primitive sets of a descriptor object -- spheres, triangles, meshes -- into p; sph, tri and meshes are the storage p then points into.
// `who` names the caller in the TypeError.  false: thrown.
static bool read_sets(napi_env env, napi_value d, const char* who, mirt_pass_desc& p, mirt_grid& sph, mirt_grid& tri, std::vector<mirt_grid>& meshes) {
    const auto bad = [&](const char* what) { throw_type(env, (std::string(who) + ": " + what).c_str()); return false; };
    napi_value v;
    if (prop(env, d, "spheres", &v)) { if (!read_grid(env, v, &sph)) return bad("spheres"); p.spheres = &sph; }
    if (prop(env, d, "triangles", &v)) { if (!read_grid(env, v, &tri)) return bad("triangles"); p.triangles = &tri; }
    if (prop(env, d, "meshes", &v)) {
        uint32_t n = 0;
        napi_get_array_length(env, v, &n);
        meshes.resize(n);
        for (uint32_t i = 0; i < n; ++i) { napi_value e; napi_get_element(env, v, i, &e); if (!read_grid(env, e, &meshes[i])) return bad("meshes[i]"); }
    }
    p.n_meshes = (uint32_t)meshes.size();
    p.meshes = meshes.data();
    return true;
}
// ... and its lights: [{shadow, scene, light}], 16 floats each
static bool read_lights(napi_env env, napi_value d, const char* who, mirt_pass_desc& p, std::vector<mirt_light>& lights) {
    napi_value v;
    if (prop(env, d, "lights", &v)) {
        uint32_t n = 0;
        napi_get_array_length(env, v, &n);
        lights.resize(n);
        for (uint32_t i = 0; i < n; ++i) {
            napi_value e;
            napi_get_element(env, v, i, &e);
            if (!prop_floats(env, e, "shadow", lights[i].shadow, 16) || !prop_floats(env, e, "scene", lights[i].scene, 16) || !prop_floats(env, e, "light", lights[i].light, 16)) {
                throw_type(env, (std::string(who) + ": lights[i] needs shadow/scene/light (16 floats each)").c_str());
                return false;
            }
        }
    }
    p.n_lights = (uint32_t)lights.size();
    p.lights = lights.data();
    return true;
}
enum RenderCall { CALL_PASS, CALL_GUIDES, CALL_FIRST_PASS_GUIDED, CALL_PASSES_GUIDED, CALL_AO };
static napi_value render_call(napi_env env, napi_value ctxv, napi_value d, RenderCall call, napi_value nhv, napi_value adv) {
    const bool guides = call != CALL_PASS;
    void* c;
    if (!get_ext(env, ctxv, &c)) return throw_type(env, call == CALL_AO ? "renderAo(ctx, desc, aoDesc, aoOut)" : call == CALL_GUIDES ? "renderGuides(ctx, desc, normalHits, albedoDepth)" : call == CALL_FIRST_PASS_GUIDED ? "renderFirstPassGuided(ctx, desc, normalHits, albedoDepth)" : call == CALL_PASSES_GUIDED ? "renderPassesGuided(ctx, desc, normalHits, albedoDepth)" : "renderPass(ctx, desc)");
    mirt_pass_desc p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    p.bounces = 5;
    p.pass_index = 1;
    if (!prop_u32(env, d, "width", &p.width) || !prop_u32(env, d, "height", &p.height) || !prop_u32(env, d, "raysPerPixel", &p.rays_per_pixel))
        return throw_type(env, "renderPass: width/height/raysPerPixel");
    prop_u32(env, d, "row0", &p.row0);
    prop_u32(env, d, "nrows", &p.nrows);
    prop_u32(env, d, "bounces", &p.bounces);
    prop_u32(env, d, "passIndex", &p.pass_index);
    if (!prop_floats(env, d, "cam", p.cam, 16) || !prop_floats(env, d, "sceneBounds", p.scene_bounds, 8) ||
        !prop_f32(env, d, "focalLength", &p.focal_length) || !prop_f32(env, d, "lensRad", &p.lens_rad))
        return throw_type(env, "renderPass: cam (16 floats), sceneBounds (8 floats), focalLength, lensRad");
    mirt_grid sph, tri;
    std::vector<mirt_grid> meshes;
    std::vector<mirt_light> lights;
    if (!read_sets(env, d, "renderPass", p, sph, tri, meshes) || !read_lights(env, d, "renderPass", p, lights)) return nullptr;
    p.material = prop_buf(env, d, "material");
    p.seeds = prop_buf(env, d, "seeds");
    p.acu = prop_buf(env, d, "acu");
    p.pixel = prop_buf(env, d, "pixel");
    p.radiance = prop_buf(env, d, "radiance");
    bool first = false;   // desc.firstPass: initAcu folded into the pass (mirt_render_first_pass)
    { napi_value v; bool has = false; if (napi_has_named_property(env, d, "firstPass", &has) == napi_ok && has && napi_get_named_property(env, d, "firstPass", &v) == napi_ok) napi_get_value_bool(env, v, &first); }
    bool every = false;
    { napi_value v; bool has = false; if (napi_has_named_property(env, d, "everyPass", &has) == napi_ok && has && napi_get_named_property(env, d, "everyPass", &v) == napi_ok) napi_get_value_bool(env, v, &every); }
    uint32_t n_passes = 0;
    if (call == CALL_AO) {
        mirt_ao_desc a = {(uint32_t)sizeof(mirt_ao_desc), MIRT_AO_DEFAULT_SAMPLES, INFINITY, MIRT_AO_DEFAULT_BIAS};
        napi_valuetype t = napi_undefined;
        if (nhv && napi_typeof(env, nhv, &t) == napi_ok && t == napi_object) {
            prop_u32(env, nhv, "samples", &a.samples);
            prop_f32(env, nhv, "radius", &a.radius);
            prop_f32(env, nhv, "bias", &a.bias);
        }
        void* out = nullptr;
        get_ext(env, adv, &out);
        const int rc = mirt_render_ao((mirt_ctx*)c, &p, &a, (mirt_buf*)out);
        if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
        return undef(env);
    }
    if (guides) {
        void *nh = nullptr, *ad = nullptr;
        get_ext(env, nhv, &nh);
        get_ext(env, adv, &ad);
        if (call == CALL_PASSES_GUIDED && !prop_u32(env, d, "nPasses", &n_passes)) return throw_type(env, "renderPassesGuided: nPasses");
        const int rc = call == CALL_GUIDES ? mirt_render_guides((mirt_ctx*)c, &p, (mirt_buf*)nh, (mirt_buf*)ad)
                     : call == CALL_PASSES_GUIDED
                         ? mirt_render_passes_guided((mirt_ctx*)c, &p, n_passes, (first ? MIRT_PASSES_FRESH : 0u) | (every ? MIRT_PASSES_EVERY_FRAME : 0u), (mirt_buf*)nh, (mirt_buf*)ad)
                         : mirt_render_first_pass_guided((mirt_ctx*)c, &p, (mirt_buf*)nh, (mirt_buf*)ad);
        if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
        return undef(env);
    }
    int rc;
    if (prop_u32(env, d, "nPasses", &n_passes))
        rc = mirt_render_passes((mirt_ctx*)c, &p, n_passes, (first ? MIRT_PASSES_FRESH : 0u) | (every ? MIRT_PASSES_EVERY_FRAME : 0u));
    else rc = first ? mirt_render_first_pass((mirt_ctx*)c, &p) : mirt_render_pass((mirt_ctx*)c, &p);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
napi_value RenderPass(napi_env env, napi_callback_info info) {
    ARGS(2);
    return render_call(env, argv[0], argv[1], CALL_PASS, nullptr, nullptr);
}
napi_value RenderGuides(napi_env env, napi_callback_info info) {
    ARGS(4);
    return render_call(env, argv[0], argv[1], CALL_GUIDES, argv[2], argv[3]);
}
napi_value RenderAo(napi_env env, napi_callback_info info) {
    ARGS(4);
    return render_call(env, argv[0], argv[1], CALL_AO, argv[2], argv[3]);
}
napi_value AoDeferred(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "aoDeferred(ctx)");
    uint64_t n = 0;
    int rc = mirt_ao_deferred((mirt_ctx*)c, &n);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return mk_num(env, (double)n);
}
napi_value RenderFirstPassGuided(napi_env env, napi_callback_info info) {
    ARGS(4);
    return render_call(env, argv[0], argv[1], CALL_FIRST_PASS_GUIDED, argv[2], argv[3]);
}
napi_value RenderPassesGuided(napi_env env, napi_callback_info info) {
    ARGS(4);
    return render_call(env, argv[0], argv[1], CALL_PASSES_GUIDED, argv[2], argv[3]);
}

// Ray queries.  traceClosest(ctx, desc, rays, count, hits, sets): the closest hit of `count` 32-byte rays {o, mint, d, maxt} of buffer `rays`
// into hits ({normal, t, p, matId}, 32 bytes each) and / or sets (uint32 each), either may be null (mirt_trace_closest).
// traceOccluded(ctx, desc, rays, count, occluded): a byte per ray (mirt_trace_occluded).  Of desc only spheres, triangles and meshes are read.
// traceDeferred(ctx) -> how many rays the last of them re-ran in the exact kernel (mirt_trace_deferred).
static napi_value trace_call(napi_env env, napi_value* argv, bool any) {
    void *c, *rays = nullptr, *o0 = nullptr, *o1 = nullptr;
    double count = 0;
    if (!get_ext(env, argv[0], &c) || !get_f64(env, argv[3], &count) || !(count >= 0) || count > 18446744073709549568.0)
        return throw_type(env, any ? "traceOccluded(ctx, desc, rays, count, occluded)" : "traceClosest(ctx, desc, rays, count, hits, sets)");
    get_ext(env, argv[2], &rays);
    get_ext(env, argv[4], &o0);
    if (!any) get_ext(env, argv[5], &o1);
    mirt_pass_desc p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    mirt_grid sph, tri;
    std::vector<mirt_grid> meshes;
    if (!read_sets(env, argv[1], "trace", p, sph, tri, meshes)) return nullptr;
    const int rc = any ? mirt_trace_occluded((mirt_ctx*)c, &p, (mirt_buf*)rays, (uint64_t)count, (mirt_buf*)o0)
                       : mirt_trace_closest((mirt_ctx*)c, &p, (mirt_buf*)rays, (uint64_t)count, (mirt_buf*)o0, (mirt_buf*)o1);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
napi_value TraceClosest(napi_env env, napi_callback_info info) {
    ARGS(6);
    return trace_call(env, argv, false);
}
napi_value TraceOccluded(napi_env env, napi_callback_info info) {
    ARGS(5);
    return trace_call(env, argv, true);
}
napi_value TraceDeferred(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "traceDeferred(ctx)");
    uint64_t n = 0;
    int rc = mirt_trace_deferred((mirt_ctx*)c, &n);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return mk_num(env, (double)n);
}

// Path radiance of the caller's own rays.  traceRadiance(ctx, desc, radDesc, rays, count, seeds, radiance): the pass's path from each of `count`
// 32-byte rays on, radDesc = {samples, flags} (left out: 1, 0) -- seeds (int32 per ray) advanced in place, radiance the float4 accumulator per ray
// (mirt_trace_radiance).  Of desc the sets, lights, material and bounces (left out: 5) are read.  radianceDeferred(ctx) -> how many rays the last
// call re-ran in the exact kernel (mirt_radiance_deferred).
napi_value TraceRadiance(napi_env env, napi_callback_info info) {
    ARGS(7);
    void *c, *rays = nullptr, *seeds = nullptr, *radiance = nullptr;
    double count = 0;
    if (!get_ext(env, argv[0], &c) || !get_f64(env, argv[4], &count) || !(count >= 0) || count > 18446744073709549568.0)
        return throw_type(env, "traceRadiance(ctx, desc, radDesc, rays, count, seeds, radiance)");
    get_ext(env, argv[3], &rays);
    get_ext(env, argv[5], &seeds);
    get_ext(env, argv[6], &radiance);
    mirt_pass_desc p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    p.bounces = 5;
    prop_u32(env, argv[1], "bounces", &p.bounces);
    mirt_grid sph, tri;
    std::vector<mirt_grid> meshes;
    std::vector<mirt_light> lights;
    if (!read_sets(env, argv[1], "traceRadiance", p, sph, tri, meshes) || !read_lights(env, argv[1], "traceRadiance", p, lights)) return nullptr;
    p.material = prop_buf(env, argv[1], "material");
    mirt_radiance_desc rd = {(uint32_t)sizeof(mirt_radiance_desc), 1u, 0u, 0u};
    napi_valuetype t = napi_undefined;
    if (napi_typeof(env, argv[2], &t) == napi_ok && t == napi_object) {
        prop_u32(env, argv[2], "samples", &rd.samples);
        prop_u32(env, argv[2], "flags", &rd.flags);
    }
    const int rc = mirt_trace_radiance((mirt_ctx*)c, &p, &rd, (mirt_buf*)rays, (uint64_t)count, (mirt_buf*)seeds, (mirt_buf*)radiance);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
napi_value RadianceDeferred(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "radianceDeferred(ctx)");
    uint64_t n = 0;
    int rc = mirt_radiance_deferred((mirt_ctx*)c, &n);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return mk_num(env, (double)n);
}

// Panoramic, fisheye and orthographic cameras.  viewDesc = {model, width, height, k, row0, nrows, flags, eye, right, up, forward (Float32Array of
// 3 each, used as given), halfW, halfH, halfAngle, tMin, tMax, tone} -- left out: model 0, k 1, the whole image, no flags, half extents 1,
// halfAngle pi / 2, tMin 0, tMax +Infinity, tone 1.  viewRays(ctx, viewDesc, rays): the tile's 32-byte rays (mirt_view_rays).
// renderView(ctx, desc, viewDesc, seeds, radiance, pixel): the frame in one launch (mirt_render_view) -- seeds (int32 per tile ray) advanced in
// place, radiance (float4 per tile pixel) and / or pixel (RGBA8), either may be null; of desc the sets, lights, material and bounces (left out: 5)
// are read.  viewDeferred(ctx) -> how many rays the last renderView re-ran in the exact kernel, in whole blocks (mirt_view_deferred).
static bool read_view(napi_env env, napi_value d, const char* who, mirt_view_desc& v, bool with_basis = true) {
    memset(&v, 0, sizeof v);
    v.struct_size = sizeof v;
    v.k = 1u;
    v.half_w = 1.0f; v.half_h = 1.0f; v.half_angle = 0x1.921fb6p+0f; v.t_min = 0.0f; v.t_max = INFINITY; v.tone = 1.0f;
    napi_valuetype t = napi_undefined;
    if (napi_typeof(env, d, &t) != napi_ok || t != napi_object || !prop_u32(env, d, "width", &v.width) || !prop_u32(env, d, "height", &v.height)) {
        throw_type(env, (std::string(who) + ": the view needs width and height").c_str());
        return false;
    }
    if (with_basis && (!prop_floats(env, d, "eye", v.eye, 3) || !prop_floats(env, d, "right", v.right, 3) || !prop_floats(env, d, "up", v.up, 3) || !prop_floats(env, d, "forward", v.forward, 3))) {
        throw_type(env, (std::string(who) + ": the view needs width, height and eye / right / up / forward (Float32Array of 3 each)").c_str());
        return false;
    }
    prop_u32(env, d, "model", &v.model); prop_u32(env, d, "k", &v.k); prop_u32(env, d, "row0", &v.row0); prop_u32(env, d, "nrows", &v.nrows); prop_u32(env, d, "flags", &v.flags);
    prop_f32(env, d, "halfW", &v.half_w); prop_f32(env, d, "halfH", &v.half_h); prop_f32(env, d, "halfAngle", &v.half_angle);
    prop_f32(env, d, "tMin", &v.t_min); prop_f32(env, d, "tMax", &v.t_max); prop_f32(env, d, "tone", &v.tone);
    return true;
}
napi_value ViewRays(napi_env env, napi_callback_info info) {
    ARGS(3);
    void *c, *rays = nullptr;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "viewRays(ctx, viewDesc, rays)");
    get_ext(env, argv[2], &rays);
    mirt_view_desc v;
    if (!read_view(env, argv[1], "viewRays", v)) return nullptr;
    const int rc = mirt_view_rays((mirt_ctx*)c, &v, (mirt_buf*)rays);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
// viewGuides(ctx, desc, viewDesc, normalHits, albedoDepth): the first-hit guides of the tile (mirt_view_guides), float4 per tile pixel each, either
// may be null.  renderViewGuided(ctx, desc, viewDesc, seeds, radiance, pixel, normalHits, albedoDepth): the frame and its guides in one call
// (mirt_render_view_guided).  ctxGuidedViews(ctx) -> the calls whose frame launch wrote the guides itself (mirt_ctx_guided_views).
enum ViewCall { VIEW_GUIDES, VIEW_FRAME_GUIDED };
static napi_value view_call(napi_env env, napi_value* argv, ViewCall call) {
    const char* const who = call == VIEW_GUIDES ? "viewGuides" : "renderViewGuided";
    void *c, *seeds = nullptr, *radiance = nullptr, *pixel = nullptr, *nh = nullptr, *ad = nullptr;
    if (!get_ext(env, argv[0], &c))
        return throw_type(env, call == VIEW_GUIDES ? "viewGuides(ctx, desc, viewDesc, normalHits, albedoDepth)"
                                                   : "renderViewGuided(ctx, desc, viewDesc, seeds, radiance, pixel, normalHits, albedoDepth)");
    if (call == VIEW_GUIDES) {
        get_ext(env, argv[3], &nh);
        get_ext(env, argv[4], &ad);
    } else {
        get_ext(env, argv[3], &seeds);
        get_ext(env, argv[4], &radiance);
        get_ext(env, argv[5], &pixel);
        get_ext(env, argv[6], &nh);
        get_ext(env, argv[7], &ad);
    }
    mirt_pass_desc p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    p.bounces = 5;
    prop_u32(env, argv[1], "bounces", &p.bounces);
    mirt_grid sph, tri;
    std::vector<mirt_grid> meshes;
    std::vector<mirt_light> lights;
    if (!read_sets(env, argv[1], who, p, sph, tri, meshes) || (call != VIEW_GUIDES && !read_lights(env, argv[1], who, p, lights))) return nullptr;
    p.material = prop_buf(env, argv[1], "material");
    mirt_view_desc v;
    if (!read_view(env, argv[2], who, v)) return nullptr;
    const int rc = call == VIEW_GUIDES ? mirt_view_guides((mirt_ctx*)c, &p, &v, (mirt_buf*)nh, (mirt_buf*)ad)
                                       : mirt_render_view_guided((mirt_ctx*)c, &p, &v, (mirt_buf*)seeds, (mirt_buf*)radiance, (mirt_buf*)pixel, (mirt_buf*)nh, (mirt_buf*)ad);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
napi_value ViewGuides(napi_env env, napi_callback_info info) {
    ARGS(5);
    return view_call(env, argv, VIEW_GUIDES);
}
napi_value RenderViewGuided(napi_env env, napi_callback_info info) {
    ARGS(8);
    return view_call(env, argv, VIEW_FRAME_GUIDED);
}
napi_value CtxGuidedViews(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "ctxGuidedViews(ctx)");
    uint64_t n = 0;
    int rc = mirt_ctx_guided_views((mirt_ctx*)c, &n);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return mk_num(env, (double)n);
}
// viewAo(ctx, desc, viewDesc, aoDesc, seeds, aoOut): ambient occlusion of the tile (mirt_view_ao) -- of desc the primitive sets alone are read,
// aoDesc = {samples, radius, bias} as for renderAo, seeds (int32 per tile ray) read and not written, aoOut uint32 {open, cast} per tile pixel.
// viewAoDeferred(ctx) -> the pixels the last viewAo re-ran in the exact kernel (mirt_view_ao_deferred).
napi_value ViewAo(napi_env env, napi_callback_info info) {
    ARGS(6);
    void *c, *seeds = nullptr, *out = nullptr;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "viewAo(ctx, desc, viewDesc, aoDesc, seeds, aoOut)");
    get_ext(env, argv[4], &seeds);
    get_ext(env, argv[5], &out);
    mirt_pass_desc p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    mirt_grid sph, tri;
    std::vector<mirt_grid> meshes;
    if (!read_sets(env, argv[1], "viewAo", p, sph, tri, meshes)) return nullptr;
    mirt_view_desc v;
    if (!read_view(env, argv[2], "viewAo", v)) return nullptr;
    mirt_ao_desc a = {(uint32_t)sizeof(mirt_ao_desc), MIRT_AO_DEFAULT_SAMPLES, INFINITY, MIRT_AO_DEFAULT_BIAS};
    napi_valuetype t = napi_undefined;
    if (napi_typeof(env, argv[3], &t) == napi_ok && t == napi_object) {
        prop_u32(env, argv[3], "samples", &a.samples);
        prop_f32(env, argv[3], "radius", &a.radius);
        prop_f32(env, argv[3], "bias", &a.bias);
    }
    const int rc = mirt_view_ao((mirt_ctx*)c, &p, &v, &a, (mirt_buf*)seeds, (mirt_buf*)out);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
napi_value ViewAoDeferred(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "viewAoDeferred(ctx)");
    uint64_t n = 0;
    int rc = mirt_view_ao_deferred((mirt_ctx*)c, &n);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return mk_num(env, (double)n);
}
napi_value RenderView(napi_env env, napi_callback_info info) {
    ARGS(6);
    void *c, *seeds = nullptr, *radiance = nullptr, *pixel = nullptr;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "renderView(ctx, desc, viewDesc, seeds, radiance, pixel)");
    get_ext(env, argv[3], &seeds);
    get_ext(env, argv[4], &radiance);
    get_ext(env, argv[5], &pixel);
    mirt_pass_desc p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    p.bounces = 5;
    prop_u32(env, argv[1], "bounces", &p.bounces);
    mirt_grid sph, tri;
    std::vector<mirt_grid> meshes;
    std::vector<mirt_light> lights;
    if (!read_sets(env, argv[1], "renderView", p, sph, tri, meshes) || !read_lights(env, argv[1], "renderView", p, lights)) return nullptr;
    p.material = prop_buf(env, argv[1], "material");
    mirt_view_desc v;
    if (!read_view(env, argv[2], "renderView", v)) return nullptr;
    const int rc = mirt_render_view((mirt_ctx*)c, &p, &v, (mirt_buf*)seeds, (mirt_buf*)radiance, (mirt_buf*)pixel);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
// Batched view cameras.  cameras: a Float32Array of 12 per frame -- eye, right, up, forward -- whose length gives the number of frames; viewDesc as
// above without eye / right / up / forward, which a batch does not read.  viewRaysBatch(ctx, viewDesc, cameras, rays): the frames' rays, frame
// after frame (mirt_view_rays_batch).  renderViewBatch(ctx, desc, viewDesc, cameras, seeds, radiance, pixel): the frames in one launch
// (mirt_render_view_batch), the buffers holding them back to back.
static bool read_cameras(napi_env env, napi_value a, const char* who, const mirt_view_camera** cams, uint32_t* n) {
    void* data = nullptr;
    size_t nb = 0;
    bool is_typed = false;
    napi_typedarray_type type = napi_uint8_array;
    size_t length = 0, offset = 0;
    napi_value buffer;
    if (napi_is_typedarray(env, a, &is_typed) != napi_ok || !is_typed || napi_get_typedarray_info(env, a, &type, &length, &data, &buffer, &offset) != napi_ok ||
        type != napi_float32_array || !get_bytes(env, a, &data, &nb) || nb % sizeof(mirt_view_camera) != 0 ||
        nb / sizeof(mirt_view_camera) > 0xFFFFFFFFull) {
        throw_type(env, (std::string(who) + ": cameras is a Float32Array of 12 per frame (eye, right, up, forward)").c_str());
        return false;
    }
    *cams = nb ? (const mirt_view_camera*)data : nullptr;
    *n = (uint32_t)(nb / sizeof(mirt_view_camera));
    return true;
}
napi_value ViewRaysBatch(napi_env env, napi_callback_info info) {
    ARGS(4);
    void *c, *rays = nullptr;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "viewRaysBatch(ctx, viewDesc, cameras, rays)");
    get_ext(env, argv[3], &rays);
    mirt_view_desc v;
    const mirt_view_camera* cams = nullptr;
    uint32_t n = 0;
    if (!read_view(env, argv[1], "viewRaysBatch", v, false) || !read_cameras(env, argv[2], "viewRaysBatch", &cams, &n)) return nullptr;
    const int rc = mirt_view_rays_batch((mirt_ctx*)c, &v, cams, n, (mirt_buf*)rays);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
napi_value RenderViewBatch(napi_env env, napi_callback_info info) {
    ARGS(7);
    void *c, *seeds = nullptr, *radiance = nullptr, *pixel = nullptr;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "renderViewBatch(ctx, desc, viewDesc, cameras, seeds, radiance, pixel)");
    get_ext(env, argv[4], &seeds);
    get_ext(env, argv[5], &radiance);
    get_ext(env, argv[6], &pixel);
    mirt_pass_desc p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    p.bounces = 5;
    prop_u32(env, argv[1], "bounces", &p.bounces);
    mirt_grid sph, tri;
    std::vector<mirt_grid> meshes;
    std::vector<mirt_light> lights;
    if (!read_sets(env, argv[1], "renderViewBatch", p, sph, tri, meshes) || !read_lights(env, argv[1], "renderViewBatch", p, lights)) return nullptr;
    p.material = prop_buf(env, argv[1], "material");
    mirt_view_desc v;
    const mirt_view_camera* cams = nullptr;
    uint32_t n = 0;
    if (!read_view(env, argv[2], "renderViewBatch", v, false) || !read_cameras(env, argv[3], "renderViewBatch", &cams, &n)) return nullptr;
    const int rc = mirt_render_view_batch((mirt_ctx*)c, &p, &v, cams, n, (mirt_buf*)seeds, (mirt_buf*)radiance, (mirt_buf*)pixel);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
// The batch's guides and ambient occlusion, the buffers holding the frames back to back.  viewGuidesBatch(ctx, desc, viewDesc, cameras,
// normalHits, albedoDepth) (mirt_view_guides_batch); renderViewGuidedBatch(ctx, desc, viewDesc, cameras, seeds, radiance, pixel, normalHits,
// albedoDepth) (mirt_render_view_guided_batch); viewAoBatch(ctx, desc, viewDesc, cameras, aoDesc, seeds, aoOut) (mirt_view_ao_batch).
static napi_value view_batch_call(napi_env env, napi_value* argv, ViewCall call) {
    const char* const who = call == VIEW_GUIDES ? "viewGuidesBatch" : "renderViewGuidedBatch";
    void *c, *seeds = nullptr, *radiance = nullptr, *pixel = nullptr, *nh = nullptr, *ad = nullptr;
    if (!get_ext(env, argv[0], &c))
        return throw_type(env, call == VIEW_GUIDES ? "viewGuidesBatch(ctx, desc, viewDesc, cameras, normalHits, albedoDepth)"
                                                   : "renderViewGuidedBatch(ctx, desc, viewDesc, cameras, seeds, radiance, pixel, normalHits, albedoDepth)");
    if (call == VIEW_GUIDES) {
        get_ext(env, argv[4], &nh);
        get_ext(env, argv[5], &ad);
    } else {
        get_ext(env, argv[4], &seeds);
        get_ext(env, argv[5], &radiance);
        get_ext(env, argv[6], &pixel);
        get_ext(env, argv[7], &nh);
        get_ext(env, argv[8], &ad);
    }
    mirt_pass_desc p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    p.bounces = 5;
    prop_u32(env, argv[1], "bounces", &p.bounces);
    mirt_grid sph, tri;
    std::vector<mirt_grid> meshes;
    std::vector<mirt_light> lights;
    if (!read_sets(env, argv[1], who, p, sph, tri, meshes) || (call != VIEW_GUIDES && !read_lights(env, argv[1], who, p, lights))) return nullptr;
    p.material = prop_buf(env, argv[1], "material");
    mirt_view_desc v;
    const mirt_view_camera* cams = nullptr;
    uint32_t n = 0;
    if (!read_view(env, argv[2], who, v, false) || !read_cameras(env, argv[3], who, &cams, &n)) return nullptr;
    const int rc = call == VIEW_GUIDES ? mirt_view_guides_batch((mirt_ctx*)c, &p, &v, cams, n, (mirt_buf*)nh, (mirt_buf*)ad)
                                       : mirt_render_view_guided_batch((mirt_ctx*)c, &p, &v, cams, n, (mirt_buf*)seeds, (mirt_buf*)radiance, (mirt_buf*)pixel,
                                                                       (mirt_buf*)nh, (mirt_buf*)ad);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
napi_value ViewGuidesBatch(napi_env env, napi_callback_info info) {
    ARGS(6);
    return view_batch_call(env, argv, VIEW_GUIDES);
}
napi_value RenderViewGuidedBatch(napi_env env, napi_callback_info info) {
    ARGS(9);
    return view_batch_call(env, argv, VIEW_FRAME_GUIDED);
}
napi_value ViewAoBatch(napi_env env, napi_callback_info info) {
    ARGS(7);
    void *c, *seeds = nullptr, *out = nullptr;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "viewAoBatch(ctx, desc, viewDesc, cameras, aoDesc, seeds, aoOut)");
    get_ext(env, argv[5], &seeds);
    get_ext(env, argv[6], &out);
    mirt_pass_desc p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    mirt_grid sph, tri;
    std::vector<mirt_grid> meshes;
    if (!read_sets(env, argv[1], "viewAoBatch", p, sph, tri, meshes)) return nullptr;
    mirt_view_desc v;
    const mirt_view_camera* cams = nullptr;
    uint32_t n = 0;
    if (!read_view(env, argv[2], "viewAoBatch", v, false) || !read_cameras(env, argv[3], "viewAoBatch", &cams, &n)) return nullptr;
    mirt_ao_desc a = {(uint32_t)sizeof(mirt_ao_desc), MIRT_AO_DEFAULT_SAMPLES, INFINITY, MIRT_AO_DEFAULT_BIAS};
    napi_valuetype t = napi_undefined;
    if (napi_typeof(env, argv[4], &t) == napi_ok && t == napi_object) {
        prop_u32(env, argv[4], "samples", &a.samples);
        prop_f32(env, argv[4], "radius", &a.radius);
        prop_f32(env, argv[4], "bias", &a.bias);
    }
    const int rc = mirt_view_ao_batch((mirt_ctx*)c, &p, &v, cams, n, &a, (mirt_buf*)seeds, (mirt_buf*)out);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
napi_value ViewDeferred(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "viewDeferred(ctx)");
    uint64_t n = 0;
    int rc = mirt_view_deferred((mirt_ctx*)c, &n);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return mk_num(env, (double)n);
}

// filterAtrous(ctx, {width,height,iterations,flags,normalPowerLog2,tone,sigmaDepth,sigmaColour, radiance,normalHits,albedoDepth, filtered?,pixel?}):
// the a-trous filter of a frame on the device (mirt_filter_atrous); a number left out is 0, a buffer left out NULL -- the library checks them all
void filter_desc(napi_env env, napi_value d, mirt_filter_desc& f) {
    memset(&f, 0, sizeof f);
    f.struct_size = sizeof f;
    prop_u32(env, d, "width", &f.width);
    prop_u32(env, d, "height", &f.height);
    prop_u32(env, d, "iterations", &f.iterations);
    prop_u32(env, d, "flags", &f.flags);
    prop_u32(env, d, "normalPowerLog2", &f.normal_power_log2);
    prop_f32(env, d, "tone", &f.tone);
    prop_f32(env, d, "sigmaDepth", &f.sigma_depth);
    prop_f32(env, d, "sigmaColour", &f.sigma_colour);
    f.radiance = prop_buf(env, d, "radiance");
    f.normal_hits = prop_buf(env, d, "normalHits");
    f.albedo_depth = prop_buf(env, d, "albedoDepth");
    f.filtered = prop_buf(env, d, "filtered");
    f.pixel = prop_buf(env, d, "pixel");
}
napi_value FilterAtrous(napi_env env, napi_callback_info info) {
    ARGS(2);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "filterAtrous(ctx, desc)");
    mirt_filter_desc f;
    filter_desc(env, argv[1], f);
    const int rc = mirt_filter_atrous((mirt_ctx*)c, &f);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
// filterAtrousRows(ctx, desc): the same descriptor read as mirt_filter_atrous_rows reads it -- height: the rows of the window the inputs hold -- and
// imageHeight, winRow0, row0, nrows beside it
napi_value FilterAtrousRows(napi_env env, napi_callback_info info) {
    ARGS(2);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "filterAtrousRows(ctx, desc)");
    mirt_filter_desc f;
    filter_desc(env, argv[1], f);
    uint32_t image_height = 0, win_row0 = 0, row0 = 0, nrows = 0;
    prop_u32(env, argv[1], "imageHeight", &image_height);
    prop_u32(env, argv[1], "winRow0", &win_row0);
    prop_u32(env, argv[1], "row0", &row0);
    prop_u32(env, argv[1], "nrows", &nrows);
    const int rc = mirt_filter_atrous_rows((mirt_ctx*)c, &f, image_height, win_row0, row0, nrows);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}

// upsampleGuided(ctx, {width,height,factor,flags,normalPowerLog2,tone,sigmaDepth, radianceLo,normalHitsLo,albedoDepthLo, normalHits,albedoDepth,
// upsampled?,pixel?}): guide-driven upsampling of a frame shaded at 1/factor resolution (mirt_upsample_guided); a number left out is 0, a buffer
// left out NULL -- the library checks them all
void upsample_desc(napi_env env, napi_value d, mirt_upsample_desc& u) {
    memset(&u, 0, sizeof u);
    u.struct_size = sizeof u;
    prop_u32(env, d, "width", &u.width);
    prop_u32(env, d, "height", &u.height);
    prop_u32(env, d, "factor", &u.factor);
    prop_u32(env, d, "flags", &u.flags);
    prop_u32(env, d, "normalPowerLog2", &u.normal_power_log2);
    prop_f32(env, d, "tone", &u.tone);
    prop_f32(env, d, "sigmaDepth", &u.sigma_depth);
    u.radiance_lo = prop_buf(env, d, "radianceLo");
    u.normal_hits_lo = prop_buf(env, d, "normalHitsLo");
    u.albedo_depth_lo = prop_buf(env, d, "albedoDepthLo");
    u.normal_hits = prop_buf(env, d, "normalHits");
    u.albedo_depth = prop_buf(env, d, "albedoDepth");
    u.upsampled = prop_buf(env, d, "upsampled");
    u.pixel = prop_buf(env, d, "pixel");
}
napi_value UpsampleGuided(napi_env env, napi_callback_info info) {
    ARGS(2);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "upsampleGuided(ctx, desc)");
    mirt_upsample_desc u;
    upsample_desc(env, argv[1], u);
    const int rc = mirt_upsample_guided((mirt_ctx*)c, &u);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
// upsampleGuidedRows(ctx, desc): the same descriptor read as mirt_upsample_guided_rows reads it, and row0, nrows, loRow0, loNrows beside it
napi_value UpsampleGuidedRows(napi_env env, napi_callback_info info) {
    ARGS(2);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "upsampleGuidedRows(ctx, desc)");
    mirt_upsample_desc u;
    upsample_desc(env, argv[1], u);
    uint32_t row0 = 0, nrows = 0, lo_row0 = 0, lo_nrows = 0;
    prop_u32(env, argv[1], "row0", &row0);
    prop_u32(env, argv[1], "nrows", &nrows);
    prop_u32(env, argv[1], "loRow0", &lo_row0);
    prop_u32(env, argv[1], "loNrows", &lo_nrows);
    const int rc = mirt_upsample_guided_rows((mirt_ctx*)c, &u, row0, nrows, lo_row0, lo_nrows);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}

// renderFrame(ctx, {assign,width,height,cam,bounds?,nSlabs?, tSize?,tPos?,tNormal?,tMindex?,tMcolor?,tSlabSize?, sSize?,sAtoms?,sMindex?,sMcolor?,sSlabSize?,
//                   pixel, rays?, aa?}): a whole Assign04 / Assign07 frame in one launch (mirt_render_frame); aa, when given: aa x aa samples a pixel, averaged
//                   in that launch (mirt_render_frame_aa)
napi_value RenderFrame(napi_env env, napi_callback_info info) {
    ARGS(2);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "renderFrame(ctx, desc)");
    napi_value d = argv[1];
    mirt_frame_desc f;
    memset(&f, 0, sizeof f);
    f.struct_size = sizeof f;
    if (!prop_u32(env, d, "assign", &f.assign) || !prop_u32(env, d, "width", &f.width) || !prop_u32(env, d, "height", &f.height) || !prop_floats(env, d, "cam", f.cam, 16))
        return throw_type(env, "renderFrame: assign, width, height, cam (16 floats)");
    prop_floats(env, d, "bounds", f.bounds, 8);
    prop_u32(env, d, "nSlabs", &f.n_slabs);
    prop_u32(env, d, "tSize", &f.t_size);
    prop_u32(env, d, "sSize", &f.s_size);
    f.t_pos = prop_buf(env, d, "tPos"); f.t_normal = prop_buf(env, d, "tNormal"); f.t_mindex = prop_buf(env, d, "tMindex"); f.t_mcolor = prop_buf(env, d, "tMcolor");
    f.t_slab_size = prop_buf(env, d, "tSlabSize");
    f.s_atoms = prop_buf(env, d, "sAtoms"); f.s_mindex = prop_buf(env, d, "sMindex"); f.s_mcolor = prop_buf(env, d, "sMcolor"); f.s_slab_size = prop_buf(env, d, "sSlabSize");
    f.pixel = prop_buf(env, d, "pixel");
    f.rays = prop_buf(env, d, "rays");
    uint32_t aa = 1;
    const bool has_aa = prop_u32(env, d, "aa", &aa);
    int rc = has_aa ? mirt_render_frame_aa((mirt_ctx*)c, &f, aa) : mirt_render_frame((mirt_ctx*)c, &f);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
napi_value CtxSetFrameFusion(napi_env env, napi_callback_info info) {
    ARGS(2);
    void* c; uint32_t on;
    if (!get_ext(env, argv[0], &c) || !get_u32(env, argv[1], &on)) return throw_type(env, "ctxSetFrameFusion(ctx, on)");
    int rc = mirt_ctx_set_frame_fusion((mirt_ctx*)c, (int)on);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
napi_value CtxFusedFrames(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "ctxFusedFrames(ctx)");
    uint64_t n = 0;
    int rc = mirt_ctx_fused_frames((mirt_ctx*)c, &n);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return mk_num(env, (double)n);
}

napi_value SeedFill(napi_env env, napi_callback_info info) {
    ARGS(5);
    void *c, *b; double first, count; uint32_t base;
    if (!get_ext(env, argv[0], &c) || !get_ext(env, argv[1], &b) || !get_f64(env, argv[2], &first) || !get_f64(env, argv[3], &count) || !get_u32(env, argv[4], &base))
        return throw_type(env, "seedFill(ctx, buf, firstRay, count, seedBase)");
    int rc = mirt_seed_fill((mirt_ctx*)c, (mirt_buf*)b, (uint64_t)first, (uint64_t)count, base);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
napi_value Zero(napi_env env, napi_callback_info info) {
    ARGS(2);
    void *c, *b;
    if (!get_ext(env, argv[0], &c) || !get_ext(env, argv[1], &b)) return throw_type(env, "zero(ctx, buf)");
    int rc = mirt_zero((mirt_ctx*)c, (mirt_buf*)b);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
// launch-bound sequences as HIP graphs (mirt.h): captureBegin(ctx), captureEnd(ctx) -> graph, graphLaunch(ctx, graph), graphRelease(graph)
napi_value CaptureBegin(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "captureBegin(ctx)");
    int rc = mirt_capture_begin((mirt_ctx*)c);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
napi_value CaptureEnd(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "captureEnd(ctx)");
    mirt_graph* g = nullptr;
    int rc = mirt_capture_end((mirt_ctx*)c, &g);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return mk_ext(env, g);
}
napi_value GraphLaunch(napi_env env, napi_callback_info info) {
    ARGS(2);
    void *c, *g;
    if (!get_ext(env, argv[0], &c) || !get_ext(env, argv[1], &g)) return throw_type(env, "graphLaunch(ctx, graph)");
    int rc = mirt_graph_launch((mirt_ctx*)c, (mirt_graph*)g);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
napi_value GraphRelease(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* g;
    if (!get_ext(env, argv[0], &g)) return throw_type(env, "graphRelease(graph)");
    int rc = mirt_graph_release((mirt_graph*)g);
    if (rc) return throw_mirt(env, rc, nullptr);
    return undef(env);
}
// gridBuild(ctx, kind, primsF64Buf, count, nSlabs, boundsFloat64Array(6)) -> {offsets, order, total}
napi_value GridBuild(napi_env env, napi_callback_info info) {
    ARGS(6);
    void *c, *pb = nullptr; uint32_t kind, count, n; void* bd; size_t nb;
    if (!get_ext(env, argv[0], &c) || !get_u32(env, argv[1], &kind) || !get_u32(env, argv[3], &count) || !get_u32(env, argv[4], &n) ||
        !get_bytes(env, argv[5], &bd, &nb) || nb < 48)
        return throw_type(env, "gridBuild(ctx, kind, primsBuf|null, count, nSlabs, Float64Array(6))");
    get_ext(env, argv[2], &pb);
    mirt_grid_build_desc d;
    memset(&d, 0, sizeof d);
    d.struct_size = sizeof d; d.kind = kind; d.count = count; d.n_slabs = n; d.prims_f64 = (mirt_buf*)pb;
    memcpy(d.bounds, bd, 48);
    mirt_buf *off = nullptr, *ord = nullptr; uint32_t total = 0;
    int rc = mirt_grid_build((mirt_ctx*)c, &d, &off, &ord, &total);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    napi_value o;
    napi_create_object(env, &o);
    napi_set_named_property(env, o, "offsets", mk_ext(env, off));
    napi_set_named_property(env, o, "order", mk_ext(env, ord));
    napi_set_named_property(env, o, "total", mk_num(env, total));
    return o;
}
// gridGatherTriangles(ctx, order, total, posF64Buf, norF64Buf|null, Int32Array ops, Float64Array vecs, padW) -> {pos, nor}
napi_value GridGatherTriangles(napi_env env, napi_callback_info info) {
    ARGS(8);
    void *c, *ord, *pb, *nb = nullptr; uint32_t total; void *ops, *vecs; size_t nops, nvecs; double pad;
    if (!get_ext(env, argv[0], &c) || !get_ext(env, argv[1], &ord) || !get_u32(env, argv[2], &total) || !get_ext(env, argv[3], &pb) ||
        !get_bytes(env, argv[5], &ops, &nops) || !get_bytes(env, argv[6], &vecs, &nvecs) || !get_f64(env, argv[7], &pad))
        return throw_type(env, "gridGatherTriangles(ctx, order, total, posBuf, norBuf|null, Int32Array, Float64Array, padW)");
    get_ext(env, argv[4], &nb);
    const uint32_t nsteps = (uint32_t)(nops / 4);
    if (nvecs < (size_t)nsteps * 24) return throw_type(env, "gridGatherTriangles: 3 doubles per step");
    mirt_buf *po = nullptr, *no = nullptr;
    int rc = mirt_grid_gather_triangles((mirt_ctx*)c, (mirt_buf*)ord, total, (mirt_buf*)pb, (mirt_buf*)nb, nsteps, (const int32_t*)ops, (const double*)vecs,
                                        (float)pad, &po, nb ? &no : nullptr);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    napi_value o;
    napi_create_object(env, &o);
    napi_set_named_property(env, o, "pos", mk_ext(env, po));
    if (no) napi_set_named_property(env, o, "nor", mk_ext(env, no));
    return o;
}
napi_value GridGather1(napi_env env, napi_callback_info info, bool spheres) {
    ARGS(4);
    void *c, *ord, *in; uint32_t total;
    if (!get_ext(env, argv[0], &c) || !get_ext(env, argv[1], &ord) || !get_u32(env, argv[2], &total) || !get_ext(env, argv[3], &in))
        return throw_type(env, "gridGather{Spheres,U32}(ctx, order, total, inBuf)");
    mirt_buf* out = nullptr;
    int rc = spheres ? mirt_grid_gather_spheres((mirt_ctx*)c, (mirt_buf*)ord, total, (mirt_buf*)in, &out)
                     : mirt_grid_gather_u32((mirt_ctx*)c, (mirt_buf*)ord, total, (mirt_buf*)in, &out);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return mk_ext(env, out);
}
napi_value GridGatherSpheres(napi_env env, napi_callback_info info) { return GridGather1(env, info, true); }
napi_value GridGatherU32(napi_env env, napi_callback_info info) { return GridGather1(env, info, false); }

napi_value TimerStart(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "timerStart(ctx)");
    int rc = mirt_timer_start((mirt_ctx*)c);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}
napi_value TimerStopMs(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* c;
    if (!get_ext(env, argv[0], &c)) return throw_type(env, "timerStopMs(ctx)");
    float ms = 0;
    int rc = mirt_timer_stop_ms((mirt_ctx*)c, &ms);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return mk_num(env, ms);
}

// meshIngest(ctx, {nVertices, nCorners, firstCorner, model: Float32Array(16), normalMat: Float32Array(9), positions, normals, indices?}, posOut, norOut, bounds)
napi_value MeshIngest(napi_env env, napi_callback_info info) {
    ARGS(5);
    void *c, *po, *no, *bo;
    if (!get_ext(env, argv[0], &c) || !get_ext(env, argv[2], &po) || !get_ext(env, argv[3], &no) || !get_ext(env, argv[4], &bo))
        return throw_type(env, "meshIngest(ctx, desc, posOut, norOut, bounds)");
    mirt_mesh_ingest_desc d;
    memset(&d, 0, sizeof d);
    d.struct_size = sizeof d;
    if (!prop_u32(env, argv[1], "nVertices", &d.n_vertices) || !prop_u32(env, argv[1], "nCorners", &d.n_corners) || !prop_u32(env, argv[1], "firstCorner", &d.first_corner) ||
        !prop_floats(env, argv[1], "model", d.model, 16) || !prop_floats(env, argv[1], "normalMat", d.normal_mat, 9))
        return throw_type(env, "meshIngest: desc needs nVertices, nCorners, firstCorner, model (16 floats), normalMat (9 floats)");
    d.positions_f64 = prop_buf(env, argv[1], "positions");
    d.normals_f64 = prop_buf(env, argv[1], "normals");
    d.indices_u32 = prop_buf(env, argv[1], "indices");
    int rc = mirt_mesh_ingest((mirt_ctx*)c, &d, (mirt_buf*)po, (mirt_buf*)no, (mirt_buf*)bo);
    if (rc) return throw_mirt(env, rc, (mirt_ctx*)c);
    return undef(env);
}

// ---- device groups: mirt_group_create / _ctx / _destroy / _finish, mirt_tile_rows, mirt_gather -----------------------------
napi_value GroupCreate(napi_env env, napi_callback_info info) {
    ARGS(1);
    uint32_t n = 0;
    if (napi_get_array_length(env, argv[0], &n) != napi_ok || n == 0) return throw_type(env, "groupCreate([device indices])");
    std::vector<int> ids(n);
    for (uint32_t i = 0; i < n; ++i) {
        napi_value e; uint32_t d;
        if (napi_get_element(env, argv[0], i, &e) != napi_ok || !get_u32(env, e, &d)) return throw_type(env, "groupCreate: device indices are integers");
        ids[i] = (int)d;
    }
    mirt_group* g = nullptr;
    int rc = mirt_group_create(ids.data(), (int)n, &g);
    if (rc) return throw_mirt(env, rc, nullptr);
    return mk_ext(env, g);
}
napi_value GroupCtx(napi_env env, napi_callback_info info) {
    ARGS(2);
    void* g; uint32_t i;
    if (!get_ext(env, argv[0], &g) || !get_u32(env, argv[1], &i)) return throw_type(env, "groupCtx(group, index)");
    mirt_ctx* c = mirt_group_ctx((mirt_group*)g, (int)i);
    if (!c) return throw_mirt(env, MIRT_E_ARG, nullptr);
    return mk_ext(env, c);
}
napi_value GroupDestroy(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* g;
    if (!get_ext(env, argv[0], &g)) return throw_type(env, "groupDestroy(group)");
    int rc = mirt_group_destroy((mirt_group*)g);
    if (rc) return throw_mirt(env, rc, nullptr);
    return undef(env);
}
napi_value GroupFinish(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* g;
    if (!get_ext(env, argv[0], &g)) return throw_type(env, "groupFinish(group)");
    int rc = mirt_group_finish((mirt_group*)g);
    if (rc) return throw_mirt(env, rc, nullptr);
    return undef(env);
}
napi_value TileRows(napi_env env, napi_callback_info info) {
    ARGS(3);
    uint32_t h, n, i, r0 = 0, nr = 0;
    if (!get_u32(env, argv[0], &h) || !get_u32(env, argv[1], &n) || !get_u32(env, argv[2], &i)) return throw_type(env, "tileRows(height, nTiles, index)");
    mirt_tile_rows(h, n, i, &r0, &nr);
    napi_value o;
    napi_create_object(env, &o);
    napi_set_named_property(env, o, "row0", mk_num(env, r0));
    napi_set_named_property(env, o, "nrows", mk_num(env, nr));
    return o;
}
napi_value Gather(napi_env env, napi_callback_info info) {
    ARGS(6);
    void* g; void* out; uint32_t n = 0, root = 0, use_rccl = 0;
    if (!get_ext(env, argv[0], &g) || napi_get_array_length(env, argv[1], &n) != napi_ok || !get_ext(env, argv[3], &out) ||
        !get_u32(env, argv[4], &root) || !get_u32(env, argv[5], &use_rccl))
        return throw_type(env, "gather(group, [tile buffers], [tile bytes], out, root, transport)");
    const int gsize = mirt_group_size((mirt_group*)g);
    if (gsize < 0) return throw_mirt(env, gsize, nullptr);
    if ((int)n != gsize) return throw_type(env, "gather: one tile buffer per context of the group");
    std::vector<mirt_buf*> tiles(n);
    std::vector<size_t> bytes(n);
    for (uint32_t i = 0; i < n; ++i) {
        napi_value e; void* b; double nb;
        if (napi_get_element(env, argv[1], i, &e) != napi_ok || !get_ext(env, e, &b)) return throw_type(env, "gather: tiles are buffers");
        tiles[i] = (mirt_buf*)b;
        if (napi_get_element(env, argv[2], i, &e) != napi_ok || !get_f64(env, e, &nb) || nb < 0) return throw_type(env, "gather: tile byte counts are numbers");
        bytes[i] = (size_t)nb;
    }
    int rc = mirt_gather((mirt_group*)g, tiles.data(), bytes.data(), (int)n, (mirt_buf*)out, (int)root, (int)use_rccl);
    if (rc) return throw_mirt(env, rc, mirt_group_ctx((mirt_group*)g, 0));
    return undef(env);
}

// ---- the post-process stage in row tiles: the two windows and the halo exchange (mirt_filter_window_rows, mirt_upsample_low_rows, mirt_exchange_rows)
napi_value rows_object(napi_env env, uint32_t r0, uint32_t nr) {
    napi_value o;
    napi_create_object(env, &o);
    napi_set_named_property(env, o, "row0", mk_num(env, r0));
    napi_set_named_property(env, o, "nrows", mk_num(env, nr));
    return o;
}
napi_value FilterWindowRows(napi_env env, napi_callback_info info) {
    ARGS(4);
    uint32_t v[4], r0 = 0, nr = 0;
    for (int i = 0; i < 4; ++i)
        if (!get_u32(env, argv[i], &v[i])) return throw_type(env, "filterWindowRows(imageHeight, row0, nrows, iterations)");
    mirt_filter_window_rows(v[0], v[1], v[2], v[3], &r0, &nr);
    return rows_object(env, r0, nr);
}
napi_value UpsampleLowRows(napi_env env, napi_callback_info info) {
    ARGS(4);
    uint32_t v[4], r0 = 0, nr = 0;
    for (int i = 0; i < 4; ++i)
        if (!get_u32(env, argv[i], &v[i])) return throw_type(env, "upsampleLowRows(height, factor, row0, nrows)");
    mirt_upsample_low_rows(v[0], v[1], v[2], v[3], &r0, &nr);
    return rows_object(env, r0, nr);
}
// exchangeRows(group, [source buffer | null], [{row0, nrows}], [destination buffer | null], [{row0, nrows}], rowBytes)
napi_value ExchangeRows(napi_env env, napi_callback_info info) {
    ARGS(6);
    static const char usage[] = "exchangeRows(group, [src | null], [{row0, nrows}], [dst | null], [{row0, nrows}], rowBytes)";
    void* g; uint32_t n = 0; double row_bytes = 0;
    if (!get_ext(env, argv[0], &g) || napi_get_array_length(env, argv[1], &n) != napi_ok || !get_f64(env, argv[5], &row_bytes) || row_bytes < 0) return throw_type(env, usage);
    std::vector<mirt_buf*> buf[2] = {std::vector<mirt_buf*>(n, nullptr), std::vector<mirt_buf*>(n, nullptr)};
    std::vector<uint32_t> row0[2] = {std::vector<uint32_t>(n, 0), std::vector<uint32_t>(n, 0)}, nrows[2] = {std::vector<uint32_t>(n, 0), std::vector<uint32_t>(n, 0)};
    for (int side = 0; side < 2; ++side) {
        uint32_t nb = 0, nr = 0;
        if (napi_get_array_length(env, argv[1 + 2 * side], &nb) != napi_ok || napi_get_array_length(env, argv[2 + 2 * side], &nr) != napi_ok || nb != n || nr != n) return throw_type(env, usage);
        for (uint32_t i = 0; i < n; ++i) {
            napi_value e; void* b = nullptr;
            if (napi_get_element(env, argv[1 + 2 * side], i, &e) != napi_ok) return throw_type(env, usage);
            if (get_ext(env, e, &b)) buf[side][i] = (mirt_buf*)b;      // anything else (null, undefined): no buffer
            if (napi_get_element(env, argv[2 + 2 * side], i, &e) != napi_ok || !prop_u32(env, e, "row0", &row0[side][i]) || !prop_u32(env, e, "nrows", &nrows[side][i]))
                return throw_type(env, usage);
        }
    }
    int rc = mirt_exchange_rows((mirt_group*)g, buf[0].data(), row0[0].data(), nrows[0].data(), buf[1].data(), row0[1].data(), nrows[1].data(), (int)n, (size_t)row_bytes);
    if (rc) return throw_mirt(env, rc, mirt_group_ctx((mirt_group*)g, 0));
    return undef(env);
}

// mirt_abi_version / mirt_group_peer_access / mirt_gather_route: what a first run on N real devices is diagnosed from
napi_value AbiVersion(napi_env env, napi_callback_info) { return mk_num(env, mirt_abi_version()); }
napi_value GroupPeerAccess(napi_env env, napi_callback_info info) {
    ARGS(3);
    void* g; uint32_t i, j;
    if (!get_ext(env, argv[0], &g) || !get_u32(env, argv[1], &i) || !get_u32(env, argv[2], &j)) return throw_type(env, "groupPeerAccess(group, i, j)");
    int rc = mirt_group_peer_access((const mirt_group*)g, (int)i, (int)j);
    if (rc < 0) return throw_mirt(env, rc, nullptr);
    return mk_num(env, rc);
}
napi_value GatherRoute(napi_env env, napi_callback_info info) {
    ARGS(2);
    void* g; uint32_t t;
    if (!get_ext(env, argv[0], &g) || !get_u32(env, argv[1], &t)) return throw_type(env, "gatherRoute(group, tile)");
    int rc = mirt_gather_route((const mirt_group*)g, (int)t);
    if (rc < 0) return throw_mirt(env, rc, nullptr);
    return mk_num(env, rc);
}

napi_value Init(napi_env env, napi_value exports) {
    struct { const char* name; napi_callback fn; } fns[] = {
        {"deviceCount", DeviceCount}, {"deviceName", DeviceName}, {"version", Version},
        {"ctxCreate", CtxCreate}, {"ctxDestroy", CtxDestroy}, {"finish", Finish}, {"ctxSetFusion", CtxSetFusion}, {"ctxFusedPasses", CtxFusedPasses}, {"ctxGuidedPasses", CtxGuidedPasses},
        {"bufCreate", BufCreate}, {"bufRelease", BufRelease}, {"bufSize", BufSize}, {"bufWrite", BufWrite}, {"bufRead", BufRead},
        {"programCheck", ProgramCheck}, {"programDialect", ProgramDialect}, {"kernelGet", KernelGet}, {"kernelRelease", KernelRelease}, {"kernelNumArgs", KernelNumArgs},
        {"kernelPreferredMultiple", KernelPreferredMultiple}, {"kernelSetArg", KernelSetArg}, {"enqueue", Enqueue},
        {"renderPass", RenderPass}, {"renderGuides", RenderGuides}, {"renderFirstPassGuided", RenderFirstPassGuided}, {"renderPassesGuided", RenderPassesGuided}, {"traceClosest", TraceClosest}, {"traceOccluded", TraceOccluded}, {"traceDeferred", TraceDeferred}, {"traceRadiance", TraceRadiance}, {"radianceDeferred", RadianceDeferred}, {"viewRays", ViewRays}, {"renderView", RenderView}, {"viewDeferred", ViewDeferred}, {"viewRaysBatch", ViewRaysBatch}, {"renderViewBatch", RenderViewBatch}, {"viewGuidesBatch", ViewGuidesBatch}, {"renderViewGuidedBatch", RenderViewGuidedBatch}, {"viewAoBatch", ViewAoBatch}, {"viewGuides", ViewGuides}, {"viewAo", ViewAo}, {"viewAoDeferred", ViewAoDeferred}, {"renderViewGuided", RenderViewGuided}, {"ctxGuidedViews", CtxGuidedViews}, {"filterAtrous", FilterAtrous}, {"upsampleGuided", UpsampleGuided}, {"renderFrame", RenderFrame}, {"ctxSetFrameFusion", CtxSetFrameFusion}, {"ctxFusedFrames", CtxFusedFrames}, {"gridBuild", GridBuild}, {"gridGatherTriangles", GridGatherTriangles},
        {"gridGatherSpheres", GridGatherSpheres}, {"gridGatherU32", GridGatherU32}, {"renderAo", RenderAo}, {"aoDeferred", AoDeferred}, {"seedFill", SeedFill}, {"zero", Zero}, {"timerStart", TimerStart}, {"timerStopMs", TimerStopMs},
        {"captureBegin", CaptureBegin}, {"captureEnd", CaptureEnd}, {"graphLaunch", GraphLaunch}, {"graphRelease", GraphRelease},
        {"groupCreate", GroupCreate}, {"groupCtx", GroupCtx}, {"groupDestroy", GroupDestroy}, {"groupFinish", GroupFinish}, {"tileRows", TileRows}, {"gather", Gather}, {"meshIngest", MeshIngest},
        {"abiVersion", AbiVersion}, {"groupPeerAccess", GroupPeerAccess}, {"gatherRoute", GatherRoute},
        {"filterAtrousRows", FilterAtrousRows}, {"upsampleGuidedRows", UpsampleGuidedRows}, {"filterWindowRows", FilterWindowRows}, {"upsampleLowRows", UpsampleLowRows}, {"exchangeRows", ExchangeRows},
    };
    for (auto& f : fns) {
        napi_value fn;
        napi_create_function(env, f.name, NAPI_AUTO_LENGTH, f.fn, nullptr, &fn);
        napi_set_named_property(env, exports, f.name, fn);
    }
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
