// host/webcl.js -- the WebCL 1.0 object model the reference host drives, backed by the MI355X
// runtime (mirt.node -> libmirt.so -> hand-written HIP kernels).
//
// Only what the ten code.js files of the reference touch is implemented (SURVEY.md 8b), with the
// reference's call shapes:
//   webcl.getPlatforms() -> platform.getInfo(PLATFORM_*), platform.getDevices(DEVICE_TYPE_ALL)
//   device.getInfo(DEVICE_NAME | DEVICE_TYPE)                          A10 code.js:483-498, 623-631
//   webcl.createContext(device) -> ctx.createCommandQueue()            :582, 592
//   ctx.createProgram(src); program.build(); program.getBuildInfo()    :596-606
//   program.createKernel(name); kernel.setArg(i, buffer | typedArray)  :1087-1089, 1124-1131, ...
//   kernel.getWorkGroupInfo(device, KERNEL_PREFERRED_WORK_GROUP_SIZE_MULTIPLE)   :656
//   ctx.createBuffer(flags, bytes)                                     :1083, 1117-1118, ...
//   queue.enqueueWriteBuffer / enqueueReadBuffer / enqueueNDRangeKernel / finish  :1095-1096, 1153, 1532-1533
//   release() on everything                                            :1539-1552
// plus extensions: queue.renderPass(desc), the whole executeRender() in one fused launch; queue.renderGuides(desc, normalHits, albedoDepth), the
// first-hit guide buffers of the same descriptor; queue.filterFrame(desc), the a-trous filter those guides drive; queue.upsampleFrame(desc), a frame
// shaded at 1/f resolution rebuilt at full resolution from the guides of both; webcl.createDeviceGroup(devices), N contexts
// in this one process with group.gather() to assemble row tiles on one device (RCCL); queue.gridBuild*, capture / launchGraph.
//
// There is no OpenCL compiler behind createProgram(): the kernels are built-in HIP code, looked
// up by name.  build() scans the OpenCL C text for `__kernel void NAME(` and throws, with the
// missing names as the build log, if the source asks for a kernel the runtime does not have.
"use strict";
const path = require("path");

let addon = null;
function native() {
  if (!addon) {
    try {
      // MIRT_CONTRACT=default: the addon over libmirt_default.so -- the kernels built as the reference's own host builds its program (program.build() without
      // options, A10 code.js:599: AMD's 2.5-ulp division); otherwise the correctly rounded contract (the one a CPU checker can reproduce)
      addon = require(path.join(__dirname, "..", process.env.MIRT_CONTRACT === "default" ? "mirt_default.node" : "mirt.node"));
    } catch (e) {
      throw new Error("mirt.node is not built (python -c 'import __graft_entry__ as g; g.build()'): " + e.message);
    }
    // include/mirt.h MIRT_ABI_VERSION this host was written against: an addon over an older libmirt.so would pass shifted arguments
    if (addon.abiVersion() !== 4) { const v = addon.abiVersion(); addon = null; throw new Error("libmirt.so speaks ABI " + v + ", this host 4: rebuild both"); }
  }
  return addon;
}

class WebCLException extends Error {
  constructor(name, msg) { super(msg); this.name = name; this.code = name; }
}
function wrap(f) {  // native errors -> WebCL-style exceptions
  try { return f(); } catch (e) {
    const map = { MIRT_E_ARG: "INVALID_VALUE", MIRT_E_HANDLE: "INVALID_MEM_OBJECT", MIRT_E_NAME: "INVALID_KERNEL_NAME",
                  MIRT_E_UNSET: "INVALID_KERNEL_ARGS", MIRT_E_RANGE: "INVALID_BUFFER_SIZE", MIRT_E_DEVICE: "OUT_OF_RESOURCES",
                  MIRT_E_NODEVICE: "DEVICE_NOT_FOUND", MIRT_E_DATA: "INVALID_VALUE" };
    throw new WebCLException(map[e.code] || "WEBCL_IMPLEMENTATION_FAILURE", e.message);
  }
}

const MAX_PASSES_PER_CALL = 64;   // MIRT_MAX_PASSES_PER_CALL (include/mirt.h)

// MIRT_FILTER_DEFAULT_* (include/mirt.h): the shipped parameters of queue.filterFrame
const FILTER_DEFAULTS = { iterations: 3, normalPowerLog2: 5, sigmaDepth: 0.1, sigmaColour: 1.0, demodulate: true };
// MIRT_UPSAMPLE_DEFAULT_* (include/mirt.h): the shipped parameters of queue.upsampleFrame
const UPSAMPLE_DEFAULTS = { normalPowerLog2: 5, sigmaDepth: 0.1, demodulate: true };

const C = {
  // values follow the OpenCL 1.1 / WebCL 1.0 enumerants
  PLATFORM_PROFILE: 0x0900, PLATFORM_VERSION: 0x0901, PLATFORM_NAME: 0x0902, PLATFORM_VENDOR: 0x0903, PLATFORM_EXTENSIONS: 0x0904,
  DEVICE_TYPE_CPU: 2, DEVICE_TYPE_GPU: 4, DEVICE_TYPE_ALL: 0xFFFFFFFF, DEVICE_TYPE: 0x1000, DEVICE_NAME: 0x102B,
  MEM_READ_WRITE: 1, MEM_WRITE_ONLY: 2, MEM_READ_ONLY: 4,
  PROGRAM_BUILD_STATUS: 0x1181, PROGRAM_BUILD_LOG: 0x1183, BUILD_SUCCESS: 0, BUILD_ERROR: -2,
  KERNEL_PREFERRED_WORK_GROUP_SIZE_MULTIPLE: 0x11B3,
};

class WebCLDevice {
  constructor(index) { this.index = index; }
  getInfo(what) {
    if (what === C.DEVICE_NAME) return wrap(() => native().deviceName(this.index));
    if (what === C.DEVICE_TYPE) return C.DEVICE_TYPE_GPU;
    throw new WebCLException("INVALID_VALUE", "device.getInfo: unsupported query " + what);
  }
}

class WebCLPlatform {
  getInfo(what) {
    switch (what) {
      case C.PLATFORM_NAME: return "mirt (AMD Instinct MI355X, HIP)";
      case C.PLATFORM_VENDOR: return "2015-raytracing_amd";
      case C.PLATFORM_VERSION: return "WebCL 1.0 subset over " + native().version();
      case C.PLATFORM_PROFILE: return "FULL_PROFILE";
      case C.PLATFORM_EXTENSIONS: return "mirt_render_pass";
      default: throw new WebCLException("INVALID_VALUE", "platform.getInfo: unsupported query " + what);
    }
  }
  getDevices(type) {
    const n = native().deviceCount();
    if (type !== C.DEVICE_TYPE_ALL && type !== C.DEVICE_TYPE_GPU) return [];
    const out = [];
    for (let i = 0; i < n; i++) out.push(new WebCLDevice(i));
    return out;
  }
}

class WebCLBuffer {
  constructor(ctx, bytes, flags, adopt) {
    this.ctx = ctx; this.byteLength = bytes;
    this.h = adopt || wrap(() => native().bufCreate(ctx.h, bytes, flags));   // adopt: a buffer the runtime created (grid build)
  }
  release() { if (this.h) { wrap(() => native().bufRelease(this.h)); this.h = null; } }
}

class WebCLKernel {
  constructor(program, name) {
    this.ctx = program.ctx; this.name = name;
    // kernel names collide across the reference's assignments (initTrace, meshTrace): the program's dialect picks the set
    this.h = wrap(() => native().kernelGet(this.ctx.h, program.prefix + name));
  }
  setArg(index, value) {
    if (value instanceof WebCLBuffer) {
      if (!value.h) throw new WebCLException("INVALID_MEM_OBJECT", this.name + ".setArg(" + index + "): released buffer");
      wrap(() => native().kernelSetArg(this.h, index, value.h));
    } else if (ArrayBuffer.isView(value)) {
      wrap(() => native().kernelSetArg(this.h, index, value));
    } else throw new WebCLException("INVALID_ARG_VALUE", this.name + ".setArg(" + index + "): expected a WebCLBuffer or a typed array");
  }
  getWorkGroupInfo(device, what) {
    if (what === C.KERNEL_PREFERRED_WORK_GROUP_SIZE_MULTIPLE) return wrap(() => native().kernelPreferredMultiple(this.h));
    throw new WebCLException("INVALID_VALUE", "kernel.getWorkGroupInfo: unsupported query " + what);
  }
  release() { if (this.h) { wrap(() => native().kernelRelease(this.h)); this.h = null; } }
}

class WebCLProgram {
  constructor(ctx, source) {
    this.ctx = ctx; this.source = String(source); this.status = null; this.log = "";
    // which assignment's kernel set the text asks for: 10, 7, 4, 1 (0 = an assignment that is not built)
    this.dialect = native().programDialect(this.source);
    this.prefix = { 10: "", 7: "A07:", 4: "A04:", 1: "A01:" }[this.dialect] || "";
  }
  build() {
    if (!this.dialect) {
      this.status = C.BUILD_ERROR;
      this.log = "unrecognised kernel set: only the Assign10, Assign07, Assign04 and Assign01 programs have built-in HIP kernels";
      throw new WebCLException("BUILD_PROGRAM_FAILURE", this.log);
    }
    const r = wrap(() => native().programCheck(this.ctx.h, this.source));
    // kernels of the text without a HIP counterpart (A04/A07: molTrace and the legacy raytrace) only fail when asked for
    this.log = r.missing ? "no built-in HIP kernel for: " + r.log + " (createKernel on these throws INVALID_KERNEL_NAME)" : "";
    this.status = C.BUILD_SUCCESS;
  }
  getBuildInfo(device, what) {
    if (what === C.PROGRAM_BUILD_STATUS) return this.status;
    if (what === C.PROGRAM_BUILD_LOG) return this.log;
    throw new WebCLException("INVALID_VALUE", "program.getBuildInfo: unsupported query " + what);
  }
  createKernel(name) { return new WebCLKernel(this, name); }
  release() {}
}

class WebCLCommandQueue {
  constructor(ctx) { this.ctx = ctx; }
  enqueueWriteBuffer(buf, blocking, offset, nbytes, typedArray /*, events */) {
    wrap(() => native().bufWrite(buf.h, offset, nbytes, typedArray));
  }
  enqueueReadBuffer(buf, blocking, offset, nbytes, typedArray /*, events */) {
    wrap(() => native().bufRead(buf.h, offset, nbytes, typedArray));
  }
  enqueueNDRangeKernel(kernel, dim, globalOffset, globalWS, localWS) {
    if (globalOffset) throw new WebCLException("INVALID_GLOBAL_OFFSET", "global offsets are not supported (the reference passes null)");
    wrap(() => native().enqueue(this.ctx.h, kernel.h, dim, Array.from(globalWS), localWS ? Array.from(localWS) : null));
  }
  finish() { wrap(() => native().finish(this.ctx.h)); }
  // ---- extension: record a launch-bound sequence of enqueues once, replay it as a HIP graph (mirt_capture_begin/_end, mirt_graph_launch)
  captureBegin() { wrap(() => native().captureBegin(this.ctx.h)); }
  captureEnd() { return { h: wrap(() => native().captureEnd(this.ctx.h)), release() { native().graphRelease(this.h); } }; }
  launchGraph(g) { wrap(() => native().graphLaunch(this.ctx.h, g.h)); }
  // ---- extension: one fused launch for the whole pass (mirt_render_pass) -------------------
  _passDesc(desc) {
    const g = (s) => s && { prims: s.prims.h, normals: s.normals ? s.normals.h : undefined, matid: s.matid ? s.matid.h : undefined,
                            cellOffsets: s.cellOffsets.h, bounds: s.bounds, nSlabs: s.nSlabs, meshMatId: s.meshMatId || 0 };
    return Object.assign({}, desc, {
      spheres: g(desc.spheres), triangles: g(desc.triangles), meshes: (desc.meshes || []).map(g),
      material: desc.material ? desc.material.h : undefined, seeds: desc.seeds ? desc.seeds.h : undefined, acu: desc.acu ? desc.acu.h : undefined,   // no acu: a first pass that resolves its pixels itself (mirt.h)
      pixel: desc.pixel ? desc.pixel.h : undefined, radiance: desc.radiance ? desc.radiance.h : undefined,
    });
  }
  renderPass(desc) {
    const d = this._passDesc(desc);
    wrap(() => native().renderPass(this.ctx.h, d));
  }
  // ---- extension: first-hit guide buffers of desc's row tile (mirt_render_guides): float4 per pixel, normalHits = (sum of the hit samples' normals,
  // hits), albedoDepth = (sum of their material colours, sum of their hit distances).  Either may be null, not both; desc's seeds, acu, pixel,
  // radiance and lights are not needed and nothing but the two buffers is written
  renderGuides(desc, normalHits, albedoDepth) {
    const d = this._passDesc(desc);
    wrap(() => native().renderGuides(this.ctx.h, d, normalHits ? normalHits.h : null, albedoDepth ? albedoDepth.h : null));
  }
  // ---- extension: ambient occlusion of the first hit of desc's row tile in one launch (mirt_render_ao; include/mirt.h has the definition):
  // aoDesc = {samples, radius, bias} (left out: 4, Infinity, 0.001), aoOut: uint32 {open, cast} per pixel -- per hit primary sample `samples`
  // hemisphere rays of length radius from the hit point, cast counts them, open those nothing blocks.  desc.seeds is read and not written;
  // material, lights, acu, pixel and radiance are not needed.  aoDeferred(): the pixels the last call re-ran in the exact kernel.
  hasAo() { return typeof native().renderAo === "function"; }
  renderAo(desc, aoDesc, aoOut) {
    const d = this._passDesc(desc);
    wrap(() => native().renderAo(this.ctx.h, d, aoDesc || {}, aoOut ? aoOut.h : null));
  }
  aoDeferred() { return wrap(() => native().aoDeferred(this.ctx.h)); }
  // ---- extension: ray queries on the caller's own rays (mirt_trace_closest, mirt_trace_occluded; include/mirt.h has the definition).  rays: a
  // buffer of `count` 32-byte records {o.xyz, mint, d.xyz, maxt}; hits: {normal.xyz, t, p.xyz, matId (int32)} per ray; sets: a uint32 per ray, the
  // index of the set whose primitive won (0xFFFFFFFF: none); hits or sets may be null, not both.  occluded: a byte per ray.  Of desc only
  // spheres, triangles and meshes are read.  traceDeferred(): the rays the last of these calls re-ran in the exact kernel.
  hasTrace() { return typeof native().traceClosest === "function"; }
  _setsDesc(desc) {
    const g = (s) => s && { prims: s.prims.h, normals: s.normals ? s.normals.h : undefined, matid: s.matid ? s.matid.h : undefined,
                            cellOffsets: s.cellOffsets.h, bounds: s.bounds, nSlabs: s.nSlabs, meshMatId: s.meshMatId || 0 };
    return { spheres: g(desc.spheres), triangles: g(desc.triangles), meshes: (desc.meshes || []).map(g) };
  }
  traceClosest(desc, rays, count, hits, sets) {
    const d = this._setsDesc(desc);
    wrap(() => native().traceClosest(this.ctx.h, d, rays ? rays.h : null, count, hits ? hits.h : null, sets ? sets.h : null));
  }
  traceOccluded(desc, rays, count, occluded) {
    const d = this._setsDesc(desc);
    wrap(() => native().traceOccluded(this.ctx.h, d, rays ? rays.h : null, count, occluded ? occluded.h : null));
  }
  traceDeferred() { return wrap(() => native().traceDeferred(this.ctx.h)); }
  // ---- extension: path radiance of the caller's own rays in one launch (mirt_trace_radiance; include/mirt.h has the definition): the pass's path
  // -- closest hit, lightRender, per-light shadow and shade, desc.bounces bounces (left out: 5) -- from each of `count` 32-byte rays on,
  // radDesc = {samples, flags} (left out: 1, 0; flags: RADIANCE_ACCUMULATE 1, RADIANCE_NO_EMITTERS 2).  seeds: an int32 per ray, advanced in
  // place; radiance: the float4 accumulator per ray, rgb sums and the number of contributions.  Of desc spheres, triangles, meshes, lights,
  // material and bounces are read.  radianceDeferred(): the rays the last call re-ran in the exact kernel.
  hasTraceRadiance() { return typeof native().traceRadiance === "function"; }
  traceRadiance(desc, radDesc, rays, count, seeds, radiance) {
    const d = Object.assign(this._setsDesc(desc), { lights: desc.lights || [], material: desc.material ? desc.material.h : undefined });
    if (desc.bounces !== undefined) d.bounces = desc.bounces;
    wrap(() => native().traceRadiance(this.ctx.h, d, radDesc || {}, rays ? rays.h : null, count, seeds ? seeds.h : null, radiance ? radiance.h : null));
  }
  radianceDeferred() { return wrap(() => native().radianceDeferred(this.ctx.h)); }
  // ---- extension: panoramic, fisheye and orthographic cameras (mirt_view_rays, mirt_render_view; include/mirt.h has the definition).  view =
  // {model: VIEW_ORTHOGRAPHIC 0 | VIEW_EQUIRECT 1 | VIEW_FISHEYE 2, width, height (the whole image), k (samples per axis: 1, 2, 4, 8, 16), row0, nrows
  // (left out: the whole image), flags (VIEW_ACCUMULATE 1), eye, right, up, forward (3 numbers each, used as given), halfW, halfH (ORTHOGRAPHIC),
  // halfAngle (FISHEYE, radians), tMin, tMax, tone}.  viewRays(view, rays): the tile's width * nrows * k * k 32-byte rays.  renderView(desc, view,
  // seeds, radiance, pixel): the frame in one launch -- seeds: an int32 per tile ray, advanced in place; radiance: float4 per tile pixel, the sums in
  // copyToPixel's order (continued from its contents with VIEW_ACCUMULATE); pixel: RGBA8, tone-mapped with view.tone; either output may be null.  Of
  // desc spheres, triangles, meshes, lights, material and bounces (left out: 5) are read.  viewDeferred(): the rays the last renderView re-ran in
  // the exact kernel, in whole blocks of 256.
  hasView() { return typeof native().renderView === "function"; }
  _viewDesc(view) {
    const v3 = (a) => Float32Array.from(a || []);
    return Object.assign({}, view, { eye: v3(view.eye), right: v3(view.right), up: v3(view.up), forward: v3(view.forward) });
  }
  viewRays(view, rays) { wrap(() => native().viewRays(this.ctx.h, this._viewDesc(view), rays ? rays.h : null)); }
  renderView(desc, view, seeds, radiance, pixel) {
    const d = Object.assign(this._setsDesc(desc), { lights: desc.lights || [], material: desc.material ? desc.material.h : undefined });
    if (desc.bounces !== undefined) d.bounces = desc.bounces;
    wrap(() => native().renderView(this.ctx.h, d, this._viewDesc(view), seeds ? seeds.h : null, radiance ? radiance.h : null, pixel ? pixel.h : null));
  }
  viewDeferred() { return wrap(() => native().viewDeferred(this.ctx.h)); }
  // ---- extension: batched view cameras (mirt_view_rays_batch, mirt_render_view_batch): the frames of N cameras that share everything of `view`
  // but the basis, in one launch.  cameras: 12 numbers per frame -- eye, right, up, forward -- as a Float32Array or an array; view.eye / right /
  // up / forward are not read; whole frames only (no row0 / nrows).  The buffers hold the frames back to back: frame f ends in each as after
  // viewRays / renderView on its slice with cameras[f].  viewDeferred() reports the batch as it reports renderView.
  hasViewBatch() { return typeof native().renderViewBatch === "function"; }
  _cameras(cameras) { return cameras instanceof Float32Array ? cameras : Float32Array.from(cameras || []); }
  viewRaysBatch(view, cameras, rays) { wrap(() => native().viewRaysBatch(this.ctx.h, Object.assign({}, view), this._cameras(cameras), rays ? rays.h : null)); }
  renderViewBatch(desc, view, cameras, seeds, radiance, pixel) {
    const d = Object.assign(this._setsDesc(desc), { lights: desc.lights || [], material: desc.material ? desc.material.h : undefined });
    if (desc.bounces !== undefined) d.bounces = desc.bounces;
    wrap(() => native().renderViewBatch(this.ctx.h, d, Object.assign({}, view), this._cameras(cameras), seeds ? seeds.h : null, radiance ? radiance.h : null, pixel ? pixel.h : null));
  }
  // ---- extension: the batch's guides and ambient occlusion (mirt_view_guides_batch, mirt_render_view_guided_batch, mirt_view_ao_batch): what
  // viewGuides, renderViewGuided and viewAo (below) are to one camera, for the N frames of `cameras` in one launch, the buffers holding the
  // frames back to back.  guidedViews() counts a guided batch call on the one-launch route once; viewAoDeferred() reports the last viewAoBatch.
  // hasViewBatchAov(): the loaded library has the three entry points
  hasViewBatchAov() {
    return typeof native().viewGuidesBatch === "function" && typeof native().renderViewGuidedBatch === "function" && typeof native().viewAoBatch === "function";
  }
  viewGuidesBatch(desc, view, cameras, normalHits, albedoDepth) {
    const d = Object.assign(this._setsDesc(desc), { material: desc.material ? desc.material.h : undefined });
    wrap(() => native().viewGuidesBatch(this.ctx.h, d, Object.assign({}, view), this._cameras(cameras), normalHits ? normalHits.h : null, albedoDepth ? albedoDepth.h : null));
  }
  renderViewGuidedBatch(desc, view, cameras, seeds, radiance, pixel, normalHits, albedoDepth) {
    const d = Object.assign(this._setsDesc(desc), { lights: desc.lights || [], material: desc.material ? desc.material.h : undefined });
    if (desc.bounces !== undefined) d.bounces = desc.bounces;
    wrap(() => native().renderViewGuidedBatch(this.ctx.h, d, Object.assign({}, view), this._cameras(cameras), seeds ? seeds.h : null, radiance ? radiance.h : null,
                                              pixel ? pixel.h : null, normalHits ? normalHits.h : null, albedoDepth ? albedoDepth.h : null));
  }
  viewAoBatch(desc, view, cameras, aoDesc, seeds, aoOut) {
    const d = this._setsDesc(desc);
    wrap(() => native().viewAoBatch(this.ctx.h, d, Object.assign({}, view), this._cameras(cameras), aoDesc || {}, seeds ? seeds.h : null, aoOut ? aoOut.h : null));
  }
  // ---- extension: the first-hit guides of those cameras (mirt_view_guides, mirt_render_view_guided).  viewGuides(desc, view, normalHits,
  // albedoDepth): float4 per tile pixel each, as renderGuides writes them for the thin lens -- what filterAtrous reads; either may be null; of desc
  // the sets and material are read; depth is in units of |forward| and the basis as given.  renderViewGuided(desc, view, seeds, radiance, pixel,
  // normalHits, albedoDepth): every buffer ends as after renderView then viewGuides; at k = 1, 2, 4 and 8 the frame's own launch writes the guides
  // (guidedViews() counts those calls), elsewhere the guide launches follow it.  hasViewGuides(): the loaded library has the entry points
  hasViewGuides() { return typeof native().renderViewGuided === "function" && typeof native().viewGuides === "function"; }
  viewGuides(desc, view, normalHits, albedoDepth) {
    const d = Object.assign(this._setsDesc(desc), { material: desc.material ? desc.material.h : undefined });
    wrap(() => native().viewGuides(this.ctx.h, d, this._viewDesc(view), normalHits ? normalHits.h : null, albedoDepth ? albedoDepth.h : null));
  }
  renderViewGuided(desc, view, seeds, radiance, pixel, normalHits, albedoDepth) {
    const d = Object.assign(this._setsDesc(desc), { lights: desc.lights || [], material: desc.material ? desc.material.h : undefined });
    if (desc.bounces !== undefined) d.bounces = desc.bounces;
    wrap(() => native().renderViewGuided(this.ctx.h, d, this._viewDesc(view), seeds ? seeds.h : null, radiance ? radiance.h : null, pixel ? pixel.h : null,
                                         normalHits ? normalHits.h : null, albedoDepth ? albedoDepth.h : null));
  }
  guidedViews() { return wrap(() => native().ctxGuidedViews(this.ctx.h)); }
  // ---- extension: ambient occlusion of those cameras in one launch (mirt_view_ao).  viewAo(desc, view, aoDesc, seeds, aoOut): aoDesc = {samples,
  // radius, bias} (left out: 4, Infinity, 0.001); seeds: an int32 per tile ray, read and not written; aoOut: uint32 {open, cast} per tile pixel, as
  // renderAo writes them for the thin lens.  Of desc only spheres, triangles and meshes are read.  viewAoDeferred(): the pixels the last call re-ran
  // in the exact kernel.  hasViewAo(): the loaded library has the entry point
  hasViewAo() { return typeof native().viewAo === "function"; }
  viewAo(desc, view, aoDesc, seeds, aoOut) {
    const d = this._setsDesc(desc);
    wrap(() => native().viewAo(this.ctx.h, d, this._viewDesc(view), aoDesc || {}, seeds ? seeds.h : null, aoOut ? aoOut.h : null));
  }
  viewAoDeferred() { return wrap(() => native().viewAoDeferred(this.ctx.h)); }
  // ---- extension: a frame's first pass and its guide buffers in one call (mirt_render_first_pass_guided): every buffer ends as after
  // renderPass(desc with firstPass) followed by renderGuides(desc, normalHits, albedoDepth) -- where the pass resolves its pixels at 4, 16 or 64 rays
  // per pixel the pass's own launch writes the guides (ctx.guidedPasses() counts those calls), elsewhere the guide launches follow it.
  // hasFirstPassGuided(): the loaded library has the entry point
  hasFirstPassGuided() { return typeof native().renderFirstPassGuided === "function"; }
  renderFirstPassGuided(desc, normalHits, albedoDepth) {
    const d = this._passDesc(desc);
    wrap(() => native().renderFirstPassGuided(this.ctx.h, d, normalHits ? normalHits.h : null, albedoDepth ? albedoDepth.h : null));
  }
  // ---- extension: the edge-avoiding a-trous filter of a frame on the device (mirt_filter_atrous; include/mirt.h has the definition).  desc:
  // {width, height, tone: 1 / (raysPerPixel * passes), radiance, normalHits, albedoDepth, filtered?, pixel?} plus any of iterations,
  // normalPowerLog2, sigmaDepth, sigmaColour, demodulate (webcl.FILTER_DEFAULTS where left out) and structure ("direct" | "tiled": one kernel
  // structure for every step, for measurement).  radiance as a pass writes it, the guides as renderGuides writes them; filtered: float4 per pixel,
  // un-scaled like radiance; pixel: RGBA8.  Either output may be left out, not both.  The frame is filtered whole: gather row tiles first.
  filterFrame(desc) { wrap(() => native().filterAtrous(this.ctx.h, this._filterDesc(desc))); }
  // the same filter on rows [row0, row0 + nrows) of a width x imageHeight image (mirt_filter_atrous_rows): desc as filterFrame's, read differently --
  // height: the rows the three inputs hold, image rows from winRow0 on, a window that contains webcl.filterWindowRows(imageHeight, row0, nrows,
  // iterations); filtered / pixel hold the nrows own rows alone -- plus {imageHeight, winRow0, row0, nrows}.  The bits are the whole frame's.
  filterFrameRows(desc) {
    const d = Object.assign(this._filterDesc(desc), { imageHeight: desc.imageHeight, winRow0: desc.winRow0, row0: desc.row0, nrows: desc.nrows });
    wrap(() => native().filterAtrousRows(this.ctx.h, d));
  }
  _filterDesc(desc) {
    const v = Object.assign({}, FILTER_DEFAULTS);
    for (const k of Object.keys(FILTER_DEFAULTS)) if (desc[k] !== undefined && desc[k] !== null) v[k] = desc[k];
    const h = (b) => (b ? b.h : undefined);
    const d = { width: desc.width, height: desc.height, iterations: v.iterations, normalPowerLog2: v.normalPowerLog2, sigmaDepth: v.sigmaDepth,
                sigmaColour: v.sigmaColour, tone: Math.fround(desc.tone), flags: (v.demodulate ? 1 : 0) | ({ direct: 2, tiled: 4 }[desc.structure] || 0),
                radiance: h(desc.radiance), normalHits: h(desc.normalHits), albedoDepth: h(desc.albedoDepth), filtered: h(desc.filtered), pixel: h(desc.pixel) };
    return d;
  }
  // ---- extension: guide-driven upsampling of a frame shaded at 1/factor resolution (mirt_upsample_guided; include/mirt.h has the definition).
  // desc: {width, height (the OUTPUT size, multiples of factor), factor: 2..4, tone: the low frame's 1 / (raysPerPixel * passes), radianceLo (a pass's
  // radiance or filterFrame's filtered), normalHitsLo, albedoDepthLo (renderGuides at the low size), normalHits, albedoDepth (renderGuides at the
  // output size), upsampled?, pixel?} plus any of normalPowerLog2, sigmaDepth, demodulate (webcl.UPSAMPLE_DEFAULTS where left out).  upsampled:
  // float4 per output pixel, un-scaled like radiance; pixel: RGBA8.  Either output may be left out, not both.  Whole frames: gather row tiles first.
  upsampleFrame(desc) { wrap(() => native().upsampleGuided(this.ctx.h, this._upsampleDesc(desc))); }
  // the same upsampler on output rows [row0, row0 + nrows) (mirt_upsample_guided_rows): desc as upsampleFrame's -- width, height: the whole output
  // image -- with normalHits, albedoDepth, upsampled and pixel holding those rows alone and the three low inputs the low rows [loRow0, loRow0 +
  // loNrows), a range that contains webcl.upsampleLowRows(height, factor, row0, nrows); plus {row0, nrows, loRow0, loNrows}.
  upsampleFrameRows(desc) {
    const d = Object.assign(this._upsampleDesc(desc), { row0: desc.row0, nrows: desc.nrows, loRow0: desc.loRow0, loNrows: desc.loNrows });
    wrap(() => native().upsampleGuidedRows(this.ctx.h, d));
  }
  _upsampleDesc(desc) {
    const v = Object.assign({}, UPSAMPLE_DEFAULTS);
    for (const k of Object.keys(UPSAMPLE_DEFAULTS)) if (desc[k] !== undefined && desc[k] !== null) v[k] = desc[k];
    const h = (b) => (b ? b.h : undefined);
    const d = { width: desc.width, height: desc.height, factor: desc.factor, normalPowerLog2: v.normalPowerLog2, sigmaDepth: v.sigmaDepth,
                tone: Math.fround(desc.tone), flags: v.demodulate ? 1 : 0, radianceLo: h(desc.radianceLo), normalHitsLo: h(desc.normalHitsLo),
                albedoDepthLo: h(desc.albedoDepthLo), normalHits: h(desc.normalHits), albedoDepth: h(desc.albedoDepth), upsampled: h(desc.upsampled),
                pixel: h(desc.pixel) };
    return d;
  }
  // ---- extension: a whole Assign04 / Assign07 frame in one launch (mirt_render_frame): initTrace and the trace kernel(s) on one thread per pixel,
  // no ray buffer unless desc.rays is given.  desc: {assign, width, height, cam, bounds, nSlabs, pixel, rays?} plus the mesh {tSize, tPos, tNormal,
  // tMindex, tMcolor, tSlabSize} and / or the molecule {sSize, sAtoms, sMindex, sMcolor, sSlabSize} as WebCLBuffers; both: molecule, then mesh (computeBoth)
  // desc.aa (1 to 4), when given: aa x aa samples a pixel, averaged in that launch (mirt_render_frame_aa); it rides along to the addon as it is
  renderFrame(desc) {
    const d = Object.assign({}, desc);
    for (const k of ["tPos", "tNormal", "tMindex", "tMcolor", "tSlabSize", "sAtoms", "sMindex", "sMcolor", "sSlabSize", "pixel", "rays"]) d[k] = desc[k] ? desc[k].h : undefined;
    wrap(() => native().renderFrame(this.ctx.h, d));
  }
  // n passes from desc.passIndex on in one call (mirt_render_passes): the frame after the last of them; desc.firstPass starts the frame, and then
  // desc.acu may be null where the passes resolve their own pixels (rays_per_pixel > 1 dividing 256, or above 256: mirt.h).
  // At most MAX_PASSES_PER_CALL (checked here: the addon reads the count as a uint32, which would wrap)
  // desc.everyPass: the frame after every pass too (MIRT_PASSES_EVERY_FRAME): desc.pixel / desc.radiance hold n frames back to back (checked here)
  // guides ({normalHits, albedoDepth}, either may be null, not both): the frame's guide buffers from the same call too (mirt_render_passes_guided,
  // renderPassesGuided below)
  renderPasses(desc, n, guides) {
    if (!Number.isInteger(n) || n < 1 || n > MAX_PASSES_PER_CALL)
      throw new WebCLException("INVALID_VALUE", "renderPasses: the pass count is an integer in 1.." + MAX_PASSES_PER_CALL + " (MIRT_MAX_PASSES_PER_CALL), not " + n);
    if (desc.everyPass) {
      const npix = (desc.nrows || desc.height) * desc.width;
      if (!desc.pixel && !desc.radiance) throw new WebCLException("INVALID_VALUE", "renderPasses: everyPass needs a pixel or radiance buffer for the frames");
      for (const [name, b, per] of [["pixel", desc.pixel, 4], ["radiance", desc.radiance, 16]])
        if (b && b.byteLength < n * npix * per)
          throw new WebCLException("INVALID_BUFFER_SIZE", `renderPasses: ${name} holds ${b.byteLength} bytes, ${n} frames of ${npix} pixels need ${n * npix * per}`);
    }
    if (!guides) { this.renderPass(Object.assign({}, desc, { nPasses: n })); return; }
    const d = this._passDesc(Object.assign({}, desc, { nPasses: n }));
    wrap(() => native().renderPassesGuided(this.ctx.h, d, guides.normalHits ? guides.normalHits.h : null, guides.albedoDepth ? guides.albedoDepth.h : null));
  }
  // ---- extension: n passes and the frame's guide buffers in one call (mirt_render_passes_guided): every buffer ends as after renderPasses(desc, n)
  // followed by renderGuides(desc, normalHits, albedoDepth) -- where the launch resolves its pixels at 4, 16 or 64 rays per pixel its first pass
  // writes the guides (ctx.guidedPasses() counts those calls), elsewhere the guide launches follow.  hasPassesGuided(): the addon binds the entry point (it links the library, so an addon that has it loads only beside a library that has it)
  hasPassesGuided() { return typeof native().renderPassesGuided === "function"; }
  renderPassesGuided(desc, n, normalHits, albedoDepth) { this.renderPasses(desc, n, { normalHits: normalHits, albedoDepth: albedoDepth }); }
  // ---- extension: the host's grid builders on the device (mirt_grid_build / mirt_grid_gather_*) ----
  // primsF64: a Float64Array (uploaded here) or a WebCLBuffer that already holds the fp64 soup (meshIngest) with `count` primitives
  gridBuild(kind, primsF64, bounds6, nSlabs, count) {
    const onDevice = primsF64 instanceof WebCLBuffer;
    if (!onDevice) count = primsF64.length / (kind ? 9 : 4);
    let pb = onDevice ? primsF64 : null;
    if (!onDevice && count) { pb = this.ctx.createBuffer(C.MEM_READ_WRITE, primsF64.byteLength); this.enqueueWriteBuffer(pb, false, 0, primsF64.byteLength, primsF64, []); }
    const r = wrap(() => native().gridBuild(this.ctx.h, kind, pb && count ? pb.h : null, count, nSlabs, new Float64Array(bounds6)));
    if (pb && !onDevice) pb.release();
    return { offsets: new WebCLBuffer(this.ctx, (nSlabs * nSlabs * nSlabs + 1) * 4, 0, r.offsets), order: new WebCLBuffer(this.ctx, Math.max(r.total * 4, 16), 0, r.order), total: r.total };
  }
  gridGatherTriangles(order, total, posF64, norF64, steps, padW) {
    const onDevice = posF64 instanceof WebCLBuffer;   // fp64 soups already on the device (meshIngest): used in place, left to the caller
    const up = (a) => { if (onDevice) return a; const b = this.ctx.createBuffer(C.MEM_READ_WRITE, Math.max(a.byteLength, 16)); if (a.byteLength) this.enqueueWriteBuffer(b, false, 0, a.byteLength, a, []); return b; };
    const pb = up(posF64), nb = norF64 ? up(norF64) : null;
    const ops = new Int32Array(steps.map((s) => s.op)), vecs = new Float64Array(steps.length * 3);
    steps.forEach((s, i) => vecs.set(s.v, 3 * i));
    const r = wrap(() => native().gridGatherTriangles(this.ctx.h, order.h, total, pb.h, nb ? nb.h : null, ops, vecs, padW || 0));
    if (!onDevice) { pb.release(); if (nb) nb.release(); }
    return { pos: new WebCLBuffer(this.ctx, Math.max(total * 48, 16), 0, r.pos), nor: r.nor ? new WebCLBuffer(this.ctx, Math.max(total * 48, 16), 0, r.nor) : null };
  }
  gridGatherSpheres(order, total, sphF64) {
    const b = this.ctx.createBuffer(C.MEM_READ_WRITE, Math.max(sphF64.byteLength, 16));
    if (sphF64.byteLength) this.enqueueWriteBuffer(b, false, 0, sphF64.byteLength, sphF64, []);
    const h = wrap(() => native().gridGatherSpheres(this.ctx.h, order.h, total, b.h));
    b.release();
    return new WebCLBuffer(this.ctx, Math.max(total * 16, 16), 0, h);
  }
  gridGatherU32(order, total, valuesU32) {
    const b = this.ctx.createBuffer(C.MEM_READ_WRITE, Math.max(valuesU32.byteLength, 16));
    if (valuesU32.byteLength) this.enqueueWriteBuffer(b, false, 0, valuesU32.byteLength, valuesU32, []);
    const h = wrap(() => native().gridGatherU32(this.ctx.h, order.h, total, b.h));
    b.release();
    return new WebCLBuffer(this.ctx, Math.max(total * 4, 16), 0, h);
  }
  // ---- extension: parseMeshJSON (tri/meshDataVersion1.js:12-78) on the device (mirt_mesh_ingest).  `model` is the parsed mesh file;
  // `normalFromMat4` the host's per-node 3x3 (scene.js).  Every mesh's vertex arrays go up once; each (node, mesh) pair is one launch
  // set.  Returns the fp64 soups as device buffers (feed them to gridBuild / gridGatherTriangles), the bounds and the small host arrays.
  meshIngest(model, normalFromMat4) {
    const nNodes = model.nodes ? model.nodes.length : 1;
    const cornersOf = (mesh) => (mesh.indices ? mesh.indices.length : mesh.vertexPositions.length / 3);
    let nCorners = 0;
    for (let k = 0; k < nNodes; k++) {
      const ids = model.nodes ? model.nodes[k].meshIndices : model.meshes.map((_, i) => i);
      for (const i of ids) nCorners += cornersOf(model.meshes[i]);
    }
    const mk = (bytes) => this.ctx.createBuffer(C.MEM_READ_WRITE, Math.max(bytes, 16));
    const up = (ta) => { const b = mk(ta.byteLength); if (ta.byteLength) this.enqueueWriteBuffer(b, false, 0, ta.byteLength, ta, []); return b; };
    const pos = mk(nCorners * 24), nor = mk(nCorners * 24);
    const bounds = up(new Float32Array([Infinity, Infinity, Infinity, -Infinity, -Infinity, -Infinity]));
    const uploaded = new Map();   // mesh index -> its three device arrays
    const matIdx = [];
    let first = 0;
    for (let k = 0; k < nNodes; k++) {
      const m = new Float32Array(16);   // mat4.create() + mat4.copy(): the matrix narrowed to fp32
      if (model.nodes) m.set(model.nodes[k].modelMatrix); else { m[0] = m[5] = m[10] = m[15] = 1; }
      const nm = normalFromMat4(m);
      const ids = model.nodes ? model.nodes[k].meshIndices : model.meshes.map((_, i) => i);
      for (const i of ids) {
        const mesh = model.meshes[i];
        if (!uploaded.has(i)) uploaded.set(i, { p: up(new Float64Array(mesh.vertexPositions)), n: up(new Float64Array(mesh.vertexNormals)), idx: mesh.indices ? up(new Uint32Array(mesh.indices)) : null });
        const u = uploaded.get(i), nc = cornersOf(mesh);
        wrap(() => native().meshIngest(this.ctx.h, { nVertices: mesh.vertexPositions.length / 3, nCorners: nc, firstCorner: first, model: m, normalMat: nm,
                                                       positions: u.p.h, normals: u.n.h, indices: u.idx ? u.idx.h : undefined }, pos.h, nor.h, bounds.h));
        for (let t = 0; t < nc / 3; t++) matIdx.push(mesh.materialIndex);
        first += nc;
      }
    }
    const b6 = new Float32Array(6);
    this.enqueueReadBuffer(bounds, true, 0, 24, b6, []);
    uploaded.forEach((u) => { u.p.release(); u.n.release(); if (u.idx) u.idx.release(); });
    bounds.release();
    const materials = [];
    (model.materials || []).forEach((mat) => { for (let c = 0; c < 4; c++) materials.push(mat.diffuseReflectance[c]); });
    return { nTriangles: nCorners / 3, positionsBuf: pos, normalsBuf: nor, bounds6: Array.from(b6), materialIndices: matIdx, materials: materials, nMaterials: materials.length / 4 };
  }
  seedFill(buf, firstRay, count, seedBase) { wrap(() => native().seedFill(this.ctx.h, buf.h, firstRay, count, seedBase || 0)); }
  zero(buf) { wrap(() => native().zero(this.ctx.h, buf.h)); }
  timerStart() { wrap(() => native().timerStart(this.ctx.h)); }
  timerStopMs() { return wrap(() => native().timerStopMs(this.ctx.h)); }
  release() {}
}

class WebCLContext {
  constructor(device, adopt) {
    this.device = device || new WebCLDevice(0);
    this.grouped = !!adopt;                       // a context that belongs to a device group goes with the group
    this.h = adopt || wrap(() => native().ctxCreate(this.device.index));
  }
  createCommandQueue() { return new WebCLCommandQueue(this); }
  createProgram(source) { return new WebCLProgram(this, source); }
  createBuffer(flags, bytes) { return new WebCLBuffer(this, bytes, flags); }
  // extension (mirt_ctx_set_fusion): level 2 runs a whole executeRender pass issued kernel by kernel as one fused launch.
  // DEFAULT for contexts made by webcl.createContext (below): 2.  The WebCL object model exists here for ONE host, the reference page,
  // which never reads its Ray / Poi / shadow-Ray buffers back (it cannot even size them without asking the device: code.js:1064-1076),
  // so what fusion leaves unwritten is unobservable to it and the unmodified page runs at the fused pass's speed (1080p x 16: 34.3 ->
  // 7.7 ms per pass).  ctx.setFusion(0) or MIRT_FUSION=0 in the environment restores launch-by-launch execution; the raw C ABI
  // (mirt_ctx_create) stays at 0 unless asked.
  setFusion(level) { wrap(() => native().ctxSetFusion(this.h, level)); }
  fusedPasses() { return wrap(() => native().ctxFusedPasses(this.h)); }
  // mirt_ctx_guided_passes: renderFirstPassGuided / renderPassesGuided calls whose launch wrote the guides itself
  guidedPasses() { return typeof native().ctxGuidedPasses === "function" ? wrap(() => native().ctxGuidedPasses(this.h)) : 0; }
  // extension (mirt_ctx_set_frame_fusion): the Assign04 / Assign07 pages' frame stream -- initTrace, then molTrace and / or meshTrace -- runs as one
  // launch and the Ray buffer is not written.  Off unless asked for here or with MIRT_FRAME_FUSION=1 in the environment.
  setFrameFusion(on) { wrap(() => native().ctxSetFrameFusion(this.h, on ? 1 : 0)); }
  fusedFrames() { return wrap(() => native().ctxFusedFrames(this.h)); }
  release() { if (this.h && !this.grouped) wrap(() => native().ctxDestroy(this.h)); this.h = null; }
}

// ---- extension: several devices in one process (mirt_group_*).  The reference is a single-device page; a frame shards by pixel rows
// (ray ids stay global) and the one exchange is assembling the tiles on the root device: group.gather() = RCCL over xGMI for N > 1.
class WebCLDeviceGroup {
  constructor(devices) {
    this.devices = devices;
    this.h = wrap(() => native().groupCreate(devices.map((d) => d.index)));
    this.contexts = devices.map((d, i) => new WebCLContext(d, wrap(() => native().groupCtx(this.h, i))));
  }
  tileRows(height, index) { return native().tileRows(height, this.devices.length, index); }
  // out (a buffer of contexts[root]) = the first tileBytes[i] bytes of tiles[i] (a buffer of contexts[i]), back to back
  // transport: 0 = auto (RCCL for N > 1 distinct devices, copies otherwise), 1 = RCCL, 2 = copies; `true` == 1
  gather(tiles, tileBytes, out, root, transport) {
    wrap(() => native().gather(this.h, tiles.map((b) => b.h), tileBytes, out.h, root || 0, transport === true ? 1 : (transport | 0)));
  }
  // the halo exchange (mirt_exchange_rows): src[i] (a buffer of contexts[i], or null) holds the image rows srcRows[i] = {row0, nrows} from its first
  // byte on; dst[i] (a buffer of contexts[i], or null) ends holding the image rows dstRows[i], each copied from whichever context owns it.  Ordered
  // after the work queued on the sources; complete after finish() of the destination's queue.
  exchangeRows(src, srcRows, dst, dstRows, rowBytes) {
    const hs = (a) => a.map((b) => (b ? b.h : null));
    wrap(() => native().exchangeRows(this.h, hs(src), srcRows, hs(dst), dstRows, rowBytes));
  }
  // 1 when contexts[i]'s device reads contexts[j]'s memory directly (peer access enabled at creation), 0 when copies between them are staged
  peerAccess(i, j) { return wrap(() => native().groupPeerAccess(this.h, i, j)); }
  // how the last gather() moved each tile: "none" | "rccl" | "peer" | "staged" | "local" (mirt.h MIRT_ROUTE_*)
  routes() { return this.devices.map((_, t) => ["none", "rccl", "peer", "staged", "local"][wrap(() => native().gatherRoute(this.h, t))]); }
  finish() { wrap(() => native().groupFinish(this.h)); }
  release() { if (this.h) { wrap(() => native().groupDestroy(this.h)); this.h = null; this.contexts.forEach((c) => { c.h = null; }); } }
}

const webcl = Object.assign({
  getPlatforms() { return [new WebCLPlatform()]; },
  createContext(device) {
    const c = new WebCLContext(device);
    if (process.env.MIRT_FUSION === undefined) c.setFusion(2);   // the environment, when set, has already been applied by mirt_ctx_create
    return c;
  },
  createDeviceGroup(devices) { return new WebCLDeviceGroup(devices); },
  FILTER_DEFAULTS,
  UPSAMPLE_DEFAULTS,
  // {row0, nrows}: the input rows that rows [row0, row0 + nrows) of the filtered image depend on, and the low rows that output rows [row0, row0 +
  // nrows) of the upsampler read (mirt_filter_window_rows, mirt_upsample_low_rows); {0, 0} on bad input
  filterWindowRows(imageHeight, row0, nrows, iterations) { return native().filterWindowRows(imageHeight, row0, nrows, iterations); },
  upsampleLowRows(height, factor, row0, nrows) { return native().upsampleLowRows(height, factor, row0, nrows); },
}, C);

// `window.WebCL` is only tested for existence by the reference (A10 code.js:468); `webcl` is the entry object.
module.exports = { webcl, WebCL: C, WebCLException, MAX_PASSES_PER_CALL };
