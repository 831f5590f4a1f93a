// host/renderer.js -- the render drivers of the JavaScript host.
//
// GranularRenderer is the reference's kernel plumbing, call for call: preRender() and
// executeRender() of A10 code.js:1784-1854 with the prepare*/execute* helpers (:1078-1528),
// written against the WebCL-shaped API of ./webcl.js -- same kernels, same argument indices,
// same enqueue order, same NDRange padding.  FusedRenderer asks the runtime for the same pass
// in one launch (queue.renderPass).  Both produce bit-identical frames.
"use strict";
let { webcl } = require("./webcl.js");
const { MAX_PASSES_PER_CALL } = require("./webcl.js");
const scene = require("./scene.js");
// tests point the drivers at another implementation of the same object model (./webcl_record.js) to compare call streams
function setWebCL(impl) { webcl = impl; }

const KERNELS = ["sizeofRay", "sizeofPoi", "initAcu", "initTrace", "sphereTrace", "triangleTrace", "meshTrace", "lightRender",
                 "initShadowTrace", "sphereShadowTrace", "triangleShadowTrace", "sceneRender", "bouncePaths", "copyToPixel"];
// what createProgram() is given in place of code.cl: the list of kernels this host will ask for
const MANIFEST = KERNELS.map((k) => "__kernel void " + k + "();").join("\n");

const u32 = (v) => new Uint32Array([v]);
const f32 = (v) => new Float32Array([v]);
const ceilTo = (n, m) => Math.ceil(n / m) * m;

function getLocalWS(dim, kernel, device) {  // code.js:645-672
  const m = kernel.getWorkGroupInfo(device, webcl.KERNEL_PREFERRED_WORK_GROUP_SIZE_MULTIPLE);
  if (dim === 1) return [m];
  let x = Math.floor(Math.sqrt(m));
  if (x & (x - 1)) { --x; for (let i = 1; i < 32; i <<= 1) x |= x >> i; ++x; }
  return [x, Math.floor(m / x)];
}

function pickDevice(index) {
  const devs = webcl.getPlatforms()[0].getDevices(webcl.DEVICE_TYPE_ALL);
  if (!devs.length) throw new Error("no MI355X visible: this host has no CPU path");
  return devs[index || 0];
}

// uploads the packed scene (scene.packScene) the way prepare*() do (code.js:1175-1185, 1221-1234, 1268-1278, 1375-1379)
function uploadScene(ctx, q, p) {
  const up = (a) => { const b = ctx.createBuffer(webcl.MEM_READ_ONLY, Math.max(a.byteLength, 16)); if (a.byteLength) q.enqueueWriteBuffer(b, false, 0, a.byteLength, a, []); return b; };
  const d = { bufs: [] };
  const keep = (b) => { d.bufs.push(b); return b; };
  if (p.n_spheres > 0) d.sph = { prims: keep(up(p.spheres)), matid: keep(up(p.s_matid)), cellOffsets: keep(up(p.s_box)), bounds: p.sphere_bounds, nSlabs: p.n_slabs };
  if (p.n_triangles > 0) d.tri = { prims: keep(up(p.t_pos)), normals: keep(up(p.t_normal)), matid: keep(up(p.t_matid)), cellOffsets: keep(up(p.t_box)), bounds: p.triangle_bounds, nSlabs: p.n_slabs };
  d.meshes = p.meshes.map((m) => ({ prims: keep(up(m.pos)), normals: keep(up(m.normal)), cellOffsets: keep(up(m.box)), bounds: m.bounds, nSlabs: m.nslabs, meshMatId: m.matid }));
  d.material = keep(up(p.materials));
  return d;
}

// The same device-side scene as uploadScene(), but binned ON THE DEVICE from the raw primitives (queue.gridBuild /
// gridGather*): `sc` is a scene loaded with {deferGrids: true}, `p` its packed header (camera, lights, bounds, materials).
function buildSceneOnDevice(ctx, q, sc, p) {
  const d = { bufs: [] };
  const keep = (b) => { d.bufs.push(b); return b; };
  const b6 = (b) => [b.min[0], b.min[1], b.min[2], b.max[0], b.max[1], b.max[2]];
  if (sc.spheres.length) {
    const f = new Float64Array(sc.spheres.length * 4);
    sc.spheres.forEach((s, i) => f.set([s.c.x, s.c.y, s.c.z, s.r], 4 * i));
    const g = q.gridBuild(0, f, b6(sc.sphereBounds), p.n_slabs);
    d.sph = { prims: keep(q.gridGatherSpheres(g.order, g.total, f)), matid: keep(q.gridGatherU32(g.order, g.total, new Uint32Array(sc.spheres.map((s) => s.matId)))),
              cellOffsets: keep(g.offsets), bounds: p.sphere_bounds, nSlabs: p.n_slabs };
    g.order.release();
  }
  const tri9 = (T, key) => { const f = new Float64Array(T.length * 9); T.forEach((t, i) => f.set([t[key[0]].x, t[key[0]].y, t[key[0]].z, t[key[1]].x, t[key[1]].y, t[key[1]].z, t[key[2]].x, t[key[2]].y, t[key[2]].z], 9 * i)); return f; };
  if (sc.triangles.length) {
    const pos = tri9(sc.triangles, ["p0", "p1", "p2"]), nor = tri9(sc.triangles, ["n0", "n1", "n2"]);
    const g = q.gridBuild(1, pos, b6(sc.triangleBounds), p.n_slabs);
    const t = q.gridGatherTriangles(g.order, g.total, pos, nor, [], 0);
    d.tri = { prims: keep(t.pos), normals: keep(t.nor), matid: keep(q.gridGatherU32(g.order, g.total, new Uint32Array(sc.triangles.map((x) => x.matId)))),
              cellOffsets: keep(g.offsets), bounds: p.triangle_bounds, nSlabs: p.n_slabs };
    g.order.release();
  }
  d.meshes = sc.meshes.map((m, i) => {
    // the soups are on the device already (queue.meshIngest = parseMeshJSON there) -- on the context that loaded the scene.  A row tile
    // on ANOTHER context (renderTiled: one context per device) ingests the mesh file again on its own device: buffers do not cross contexts.
    const jm = m.jmesh;
    let onDev = !!jm.positionsBuf, own = false, pos, nor;
    if (onDev && jm.positionsBuf.ctx !== ctx) {
      const r = q.meshIngest(jm.model, scene.normalFromMat4);
      pos = r.positionsBuf; nor = r.normalsBuf; own = true;
    } else if (onDev) { pos = jm.positionsBuf; nor = jm.normalsBuf; }
    else { pos = new Float64Array(jm.positions); nor = new Float64Array(jm.normals); }
    const g = q.gridBuild(1, pos, b6(m.gridBounds), m.nslabs, jm.nTriangles);      // grid on the untransformed mesh (code.js:106-112)
    const t = q.gridGatherTriangles(g.order, g.total, pos, nor, m.steps, 0);   // normalize / scale / translate in fp64, then fp32
    g.order.release();
    if (own) { pos.release(); nor.release(); }
    else if (onDev && !sc.keepSoups) { pos.release(); nor.release(); jm.positionsBuf = jm.normalsBuf = null; }
    return { prims: keep(t.pos), normals: keep(t.nor), cellOffsets: keep(g.offsets), bounds: p.meshes[i].bounds, nSlabs: m.nslabs, meshMatId: m.matId };
  });
  const mat = ctx.createBuffer(webcl.MEM_READ_ONLY, Math.max(p.materials.byteLength, 16));
  q.enqueueWriteBuffer(mat, false, 0, p.materials.byteLength, p.materials, []);
  d.material = keep(mat);
  return d;
}

class GranularRenderer {
  constructor(packed, opt) {
    opt = opt || {};
    this.p = packed;
    this.ownCtx = !opt.ctx;
    this.device = opt.ctx ? opt.ctx.device : pickDevice(opt.device);
    this.useGraph = !!opt.graph;
    this.ctx = opt.ctx || webcl.createContext(this.device);           // createCLBasicResources (code.js:576-608)
    // ours: with `fusion` the runtime runs each pass of this stream as one fused launch (webcl.createContext's default); without it this
    // renderer is the launch-by-launch path on purpose -- whoever made the context (renderFile's --device-grid hands one in)
    if (this.ctx.setFusion) this.ctx.setFusion(opt.fusion ? 2 : 0);
    this.q = this.ctx.createCommandQueue();
    this.program = this.ctx.createProgram(MANIFEST);
    this.program.build();
    this.k = {}; this.b = {}; this.gws = {}; this.lws = {};
    this.passes = 1;
    this.sceneObject = opt.sceneObject || null;
    this._preRender(opt.seeds, opt.seedBase);
  }
  _structSize(name) {  // getStructSize (code.js:1064-1076)
    const k = this.program.createKernel("sizeof" + name), b = this.ctx.createBuffer(webcl.MEM_WRITE_ONLY, 4), out = new Uint32Array(1);
    k.setArg(0, b);
    this.q.enqueueNDRangeKernel(k, 1, null, [1], [1]);
    this.q.enqueueReadBuffer(b, false, 0, 4, out, []);
    this.q.finish();
    b.release(); k.release();
    return out[0];
  }
  _preRender(seeds, seedBase) {
    const p = this.p, ctx = this.ctx, q = this.q, prog = this.program, k = this.k, b = this.b;
    const n = this.totalRays = p.rays_per_pixel * p.width * p.height;
    // prepareInitAcu
    b.acu = ctx.createBuffer(webcl.MEM_READ_WRITE, n * 16);
    const ia = prog.createKernel("initAcu");
    ia.setArg(0, b.acu); ia.setArg(1, u32(n));
    let l = getLocalWS(1, ia, this.device);
    q.enqueueNDRangeKernel(ia, 1, null, [ceilTo(n, l[0])], l);
    q.finish(); ia.release();
    // prepareInitSeeds: Math.random() in the reference; a caller-supplied array or the device-side closed form here
    b.seeds = ctx.createBuffer(webcl.MEM_READ_WRITE, n * 4);
    if (seeds) q.enqueueWriteBuffer(b.seeds, false, 0, n * 4, seeds, []); else q.seedFill(b.seeds, 0, n, seedBase || 0);
    // prepareInitTrace
    const raySize = this._structSize("Ray"), poiSize = this._structSize("Poi");
    b.rays = ctx.createBuffer(webcl.MEM_READ_WRITE, n * raySize);
    b.pois = ctx.createBuffer(webcl.MEM_READ_WRITE, n * poiSize);
    k.initTrace = prog.createKernel("initTrace");
    [b.seeds, b.rays, b.pois, p.bounds].forEach((v, i) => k.initTrace.setArg(i, v));
    k.initTrace.setArg(5, f32(p.focal_length)); k.initTrace.setArg(6, f32(p.lens_rad)); k.initTrace.setArg(7, u32(p.rays_per_pixel));
    l = this.lws.initTrace = getLocalWS(2, k.initTrace, this.device);
    this.gws.initTrace = [ceilTo(p.width, l[0]), ceilTo(p.height, l[1])];
    const d = this.dev = this.sceneObject ? buildSceneOnDevice(ctx, q, this.sceneObject, p) : uploadScene(ctx, q, p);
    if (d.sph) {  // prepareSphereTrace
      k.sphereTrace = prog.createKernel("sphereTrace");
      [u32(n), b.pois, b.rays, d.sph.prims, d.sph.matid, d.sph.cellOffsets, d.sph.bounds, u32(d.sph.nSlabs)].forEach((v, i) => k.sphereTrace.setArg(i, v));
    }
    if (d.tri) {  // prepareTriangleTrace
      k.triangleTrace = prog.createKernel("triangleTrace");
      [u32(n), b.pois, b.rays, d.tri.prims, d.tri.normals, d.tri.matid, d.tri.cellOffsets, d.tri.bounds, u32(d.tri.nSlabs)].forEach((v, i) => k.triangleTrace.setArg(i, v));
    }
    if (d.meshes.length) {  // prepareMeshTrace
      k.meshTrace = prog.createKernel("meshTrace");
      [u32(n), b.pois, b.rays].forEach((v, i) => k.meshTrace.setArg(i, v));
    }
    // prepareInitShadowTrace: asks for the Ray size again (code.js:1417-1419)
    b.shadow = ctx.createBuffer(webcl.MEM_READ_WRITE, n * this._structSize("Ray"));
    k.initShadowTrace = prog.createKernel("initShadowTrace");
    k.initShadowTrace.setArg(0, b.shadow); k.initShadowTrace.setArg(1, b.pois); k.initShadowTrace.setArg(2, u32(n)); k.initShadowTrace.setArg(4, b.seeds);
    if (d.sph) {
      k.sphereShadowTrace = prog.createKernel("sphereShadowTrace");
      [u32(n), b.shadow, d.sph.prims, d.sph.cellOffsets, d.sph.bounds, u32(d.sph.nSlabs)].forEach((v, i) => k.sphereShadowTrace.setArg(i, v));
    }
    if (d.tri || d.meshes.length) {
      k.triangleShadowTrace = prog.createKernel("triangleShadowTrace");
      k.triangleShadowTrace.setArg(0, u32(n)); k.triangleShadowTrace.setArg(1, b.shadow);
    }
    // prepareSceneRender / prepareCopyToPixel / prepareBouncePaths / prepareLightRender
    k.sceneRender = prog.createKernel("sceneRender");
    [b.acu, b.pois, b.shadow, d.material].forEach((v, i) => k.sceneRender.setArg(i, v));
    k.sceneRender.setArg(5, u32(n));
    const npix = p.width * p.height;
    b.pixel = ctx.createBuffer(webcl.MEM_WRITE_ONLY, npix * 4);
    k.copyToPixel = prog.createKernel("copyToPixel");
    k.copyToPixel.setArg(0, b.pixel); k.copyToPixel.setArg(1, b.acu); k.copyToPixel.setArg(3, u32(npix)); k.copyToPixel.setArg(4, u32(p.rays_per_pixel));
    this.gws.copyToPixel = [ceilTo(npix, 64)];
    k.bouncePaths = prog.createKernel("bouncePaths");
    [b.pois, b.rays, b.seeds, u32(n)].forEach((v, i) => k.bouncePaths.setArg(i, v));
    k.lightRender = prog.createKernel("lightRender");
    k.lightRender.setArg(0, b.pois); k.lightRender.setArg(1, b.rays); k.lightRender.setArg(2, b.acu); k.lightRender.setArg(4, u32(n));
    this.g1 = [ceilTo(n, 64)];
  }
  _run(kernel) { this.q.enqueueNDRangeKernel(kernel, 1, null, this.g1, [64]); }
  _closest() {
    const k = this.k, d = this.dev;
    if (d.sph) this._run(k.sphereTrace);
    if (d.tri) this._run(k.triangleTrace);
    for (const m of d.meshes) {  // executeMeshTrace (code.js:1293-1303)
      k.meshTrace.setArg(3, m.prims); k.meshTrace.setArg(4, m.normals); k.meshTrace.setArg(5, m.cellOffsets);
      k.meshTrace.setArg(6, u32(m.meshMatId)); k.meshTrace.setArg(7, m.bounds); k.meshTrace.setArg(8, u32(m.nSlabs));
      this._run(k.meshTrace);
    }
  }
  _direct() {
    const k = this.k, d = this.dev;
    for (const light of this.p.lights) {
      k.initShadowTrace.setArg(3, light.shadow); this._run(k.initShadowTrace);
      if (d.sph) this._run(k.sphereShadowTrace);
      const sets = (d.tri ? [d.tri] : []).concat(d.meshes);  // executeTriangleShadowTrace / executeMeshShadowTrace (code.js:1514-1528)
      for (const s of sets) {
        k.triangleShadowTrace.setArg(2, s.prims); k.triangleShadowTrace.setArg(3, s.cellOffsets); k.triangleShadowTrace.setArg(4, s.bounds);
        k.triangleShadowTrace.setArg(5, u32(s.nSlabs)); this._run(k.triangleShadowTrace);
      }
      k.sceneRender.setArg(4, light.scene); this._run(k.sceneRender);  // executeSceneRender (code.js:1402-1408)
      if (!this._recording) this.q.finish();   // the reference finishes the queue here (code.js:1406); a recording cannot wait
    }
  }
  _segments(bounces) {
    const k = this.k, p = this.p;
    k.initTrace.setArg(4, p.cam);
    this.q.enqueueNDRangeKernel(k.initTrace, 2, null, this.gws.initTrace, this.lws.initTrace);
    this._closest();
    for (const light of p.lights) { k.lightRender.setArg(3, light.light); this._run(k.lightRender); }
    this._direct();
    for (let j = 0; j < bounces; j++) { this._run(k.bouncePaths); this._closest(); this._direct(); }
  }
  // code.js:1806-1854.  opt.graph (constructor): from the second pass on the pass body -- 40-odd launches, each a few microseconds on
  // the page's 320x240 canvas -- is one HIP graph replay; copyToPixel stays outside, its scale changes every pass (code.js:1412)
  executeRender(bounces) {
    const k = this.k, p = this.p;
    bounces = bounces === undefined ? 5 : bounces;
    if (this.useGraph && this.passes > 1) {
      if (!this._graph || this._graphBounces !== bounces) {
        if (this._graph) this._graph.release();
        this.q.captureBegin();
        this._recording = true;
        try { this._segments(bounces); } finally { this._recording = false; this._graph = this.q.captureEnd(); }
        this._graphBounces = bounces;
      }
      this.q.launchGraph(this._graph);
    } else this._segments(bounces);
    k.copyToPixel.setArg(2, f32(1.0 / (p.rays_per_pixel * this.passes)));  // executeCopyToPixel (code.js:1410-1415)
    this.q.enqueueNDRangeKernel(k.copyToPixel, 1, null, this.gws.copyToPixel, [64]);
    this.passes++;
  }
  readPixels() {  // sendImagetoHTML (code.js:1530-1537)
    const out = new Uint8ClampedArray(this.p.width * this.p.height * 4);
    this.q.enqueueReadBuffer(this.b.pixel, false, 0, out.length, out, []);
    this.q.finish();
    return out;
  }
  readAcu() { const a = new Float32Array(this.totalRays * 4); this.q.enqueueReadBuffer(this.b.acu, false, 0, a.byteLength, a, []); this.q.finish(); return a; }
  release() {  // releaseCLResources (code.js:1539-1552)
    if (this._graph) { this._graph.release(); this._graph = null; }
    Object.values(this.k).forEach((k) => k.release());
    Object.values(this.b).forEach((b) => b.release());
    this.dev.bufs.forEach((b) => b.release());
    this.program.release(); this.q.release();
    if (this.ownCtx) this.ctx.release();
  }
}

class FusedRenderer {
  constructor(packed, opt) {
    opt = opt || {};
    const p = this.p = packed;
    this.ownCtx = !opt.ctx;
    this.device = opt.ctx ? opt.ctx.device : pickDevice(opt.device);
    this.ctx = opt.ctx || webcl.createContext(this.device);   // opt.ctx: a context of a device group (renderTiled)
    this.q = this.ctx.createCommandQueue();
    this.row0 = opt.row0 || 0;
    this.nrows = opt.nrows === undefined ? p.height : opt.nrows;
    this.npix = this.nrows * p.width;
    this.nrays = this.npix * p.rays_per_pixel;
    const first = this.row0 * p.width * p.rays_per_pixel;
    this.dev = opt.sceneObject ? buildSceneOnDevice(this.ctx, this.q, opt.sceneObject, p) : uploadScene(this.ctx, this.q, p);
    this.seeds = this.ctx.createBuffer(webcl.MEM_READ_WRITE, this.nrays * 4);
    if (opt.seeds) this.q.enqueueWriteBuffer(this.seeds, false, 0, this.nrays * 4, opt.seeds.subarray(first, first + this.nrays), []);
    else this.q.seedFill(this.seeds, first, this.nrays, opt.seedBase || 0);
    // not zeroed: the first pass initialises it (firstPass below).  opt.keepAcu === false: a one-pass frame without the 16 bytes per ray -- the pass
    // resolves its pixels itself (mirt_render_first_pass with acu == NULL: rays_per_pixel must divide 256 or be above 256, and there is no second
    // pass) -- or, opt.passesInOneLaunch, a frame of every pass in one call (executePasses)
    this.acu = opt.keepAcu === false ? null : this.ctx.createBuffer(webcl.MEM_READ_WRITE, this.nrays * 16);
    this.pixel = this.ctx.createBuffer(webcl.MEM_WRITE_ONLY, this.npix * 4);
    this.radiance = this.ctx.createBuffer(webcl.MEM_WRITE_ONLY, this.npix * 16);
    this.passes = 1;
  }
  passDesc(bounces) {
    const p = this.p, d = this.dev;
    return { width: p.width, height: p.height, raysPerPixel: p.rays_per_pixel, row0: this.row0, nrows: this.nrows,
      bounces: bounces === undefined ? 5 : bounces, passIndex: this.passes, cam: p.cam, sceneBounds: p.bounds,
      focalLength: p.focal_length, lensRad: p.lens_rad, spheres: d.sph, triangles: d.tri, meshes: d.meshes, lights: p.lights,
      material: d.material, seeds: this.seeds, acu: this.acu, pixel: this.pixel, radiance: this.radiance,
      firstPass: this.passes === 1 };   // preRender's initAcu (code.js:1078-1099) folded into the frame's first pass
  }
  executeRender(bounces) {
    this.q.renderPass(this.passDesc(bounces));
    this.passes++;
  }
  // n passes in one call (mirt_render_passes): the frame after the last of them, as n executeRender calls would leave it.  Starting the frame
  // it needs no accumulator where the passes resolve their own pixels (keepAcu false).  A call runs at most MAX_PASSES_PER_CALL passes: with the
  // accumulator kept, more are split into calls of that many (the frame is the same); without it a frame cannot go on after its first call
  // opt.everyPass: the frame after every pass too (MIRT_PASSES_EVERY_FRAME), into frame buffers of each call's k passes, read back after the call:
  // readFrames() returns them all.  this.pixel / this.radiance then hold the last frame, as without it.
  // opt.guided: the frame's guides too (queue.renderPassesGuided), from the first call -- they are the same for every pass of a frame.
  executePasses(n, bounces, opt) {
    const every = !!(opt && opt.everyPass);
    let guides = null;
    if (opt && opt.guided) {
      if (!this.normalHits) {
        this.normalHits = this.ctx.createBuffer(webcl.MEM_WRITE_ONLY, this.npix * 16);
        this.albedoDepth = this.ctx.createBuffer(webcl.MEM_WRITE_ONLY, this.npix * 16);
      }
      guides = { normalHits: this.normalHits, albedoDepth: this.albedoDepth };
    }
    if (!this.acu && n > MAX_PASSES_PER_CALL)
      throw new Error(`${n} passes in one launch without a per-ray accumulator: at most ${MAX_PASSES_PER_CALL} (MIRT_MAX_PASSES_PER_CALL); keep the accumulator to split them over calls`);
    if (every) this.frames = { n: 0, pixel: new Uint8ClampedArray(n * this.npix * 4), radiance: new Float32Array(n * this.npix * 4) };
    for (let left = n; left > 0; ) {
      const k = Math.min(left, MAX_PASSES_PER_CALL);
      if (!every) this.q.renderPasses(this.passDesc(bounces), k, guides);
      else {
        const fp = this.ctx.createBuffer(webcl.MEM_WRITE_ONLY, k * this.npix * 4), fr = this.ctx.createBuffer(webcl.MEM_WRITE_ONLY, k * this.npix * 16);
        try {
          this.q.renderPasses(Object.assign(this.passDesc(bounces), { pixel: fp, radiance: fr, everyPass: true }), k, guides);
          const f = this.frames, px = f.pixel.subarray(f.n * this.npix * 4, (f.n + k) * this.npix * 4), rd = f.radiance.subarray(f.n * this.npix * 4, (f.n + k) * this.npix * 4);
          this.q.enqueueReadBuffer(fp, true, 0, px.byteLength, px, []);
          this.q.enqueueReadBuffer(fr, true, 0, rd.byteLength, rd, []);
          this.q.finish();
          f.n += k;
          const last = (f.n - 1) * this.npix * 4;   // the renderer's own buffers hold the last frame
          this.q.enqueueWriteBuffer(this.pixel, true, 0, this.npix * 4, f.pixel.subarray(last, last + this.npix * 4), []);
          this.q.enqueueWriteBuffer(this.radiance, true, 0, this.npix * 16, f.radiance.subarray(last, last + this.npix * 4), []);
        } finally { fp.release(); fr.release(); }
      }
      this.passes += k;
      left -= k;
      guides = null;
    }
  }
  // n passes in one call and the frame's guides with them (queue.renderPassesGuided): executePasses(n, bounces, opt) and renderGuides() at once
  canRenderPassesGuided() { return typeof this.q.hasPassesGuided === "function" && this.q.hasPassesGuided(); }
  executePassesGuided(n, bounces, opt) { this.executePasses(n, bounces, Object.assign({}, opt, { guided: true })); }
  // first-hit guide buffers of this renderer's tile (queue.renderGuides), kept on the device for a gather: normalHits, albedoDepth, float4 per pixel
  renderGuides() {
    if (!this.normalHits) {
      this.normalHits = this.ctx.createBuffer(webcl.MEM_WRITE_ONLY, this.npix * 16);
      this.albedoDepth = this.ctx.createBuffer(webcl.MEM_WRITE_ONLY, this.npix * 16);
    }
    this.q.renderGuides(this.passDesc(), this.normalHits, this.albedoDepth);
  }
  // the frame's first pass and its guides in one call (queue.renderFirstPassGuided): executeRender() and renderGuides() at once
  canRenderGuided() { return this.passes === 1 && typeof this.q.hasFirstPassGuided === "function" && this.q.hasFirstPassGuided(); }
  executeRenderGuided(bounces) {
    if (!this.normalHits) {
      this.normalHits = this.ctx.createBuffer(webcl.MEM_WRITE_ONLY, this.npix * 16);
      this.albedoDepth = this.ctx.createBuffer(webcl.MEM_WRITE_ONLY, this.npix * 16);
    }
    this.q.renderFirstPassGuided(this.passDesc(bounces), this.normalHits, this.albedoDepth);
    this.passes++;
  }
  readGuides() {
    const n = new Float32Array(this.npix * 4), a = new Float32Array(this.npix * 4);
    this.q.enqueueReadBuffer(this.normalHits, false, 0, n.byteLength, n, []);
    this.q.enqueueReadBuffer(this.albedoDepth, false, 0, a.byteLength, a, []);
    this.q.finish();
    return { normalHits: n, albedoDepth: a };
  }
  // ambient occlusion of the first hit of this renderer's tile (queue.renderAo), from the seeds as they stand (they are not advanced): ao = any of
  // samples, radius, bias.  readAo(): Uint32Array of {open, cast} per pixel
  renderAo(ao) {
    if (!this.ao) this.ao = this.ctx.createBuffer(webcl.MEM_WRITE_ONLY, this.npix * 8);
    this.q.renderAo(this.passDesc(), ao || {}, this.ao);
  }
  readAo() {
    const o = new Uint32Array(this.npix * 2);
    this.q.enqueueReadBuffer(this.ao, false, 0, o.byteLength, o, []);
    this.q.finish();
    return o;
  }
  // the a-trous-filtered frame of this renderer's current radiance (queue.filterFrame, guided by renderGuides()'s buffers), all on the device; f: any
  // of iterations, normalPowerLog2, sigmaDepth, sigmaColour, demodulate, structure.  A row tile would be filtered alone: renderTiled gathers first
  // and filters the whole frame on the root (filterGathered)
  denoise(f, haveGuides) {   // haveGuides: renderGuides() has already run for this frame
    if (!haveGuides) this.renderGuides();
    if (!this.filtered) {
      this.filtered = this.ctx.createBuffer(webcl.MEM_WRITE_ONLY, this.npix * 16);
      this.filteredPixel = this.ctx.createBuffer(webcl.MEM_WRITE_ONLY, this.npix * 4);
    }
    this.q.filterFrame(Object.assign({}, f, { width: this.p.width, height: this.nrows, tone: 1 / (this.p.rays_per_pixel * (this.passes - 1)),
      radiance: this.radiance, normalHits: this.normalHits, albedoDepth: this.albedoDepth, filtered: this.filtered, pixel: this.filteredPixel }));
  }
  readDenoised() {
    const px = new Uint8ClampedArray(this.npix * 4), f = new Float32Array(this.npix * 4);
    this.q.enqueueReadBuffer(this.filteredPixel, false, 0, px.length, px, []);
    this.q.enqueueReadBuffer(this.filtered, false, 0, f.byteLength, f, []);
    this.q.finish();
    return { pixel: px, filtered: f };
  }
  // the frames of the last executePasses(n, bounces, {everyPass: true}): { n, pixel: n RGBA8 frames, radiance: n float4 frames }, back to back
  readFrames() { return this.frames; }
  readPixels() { const o = new Uint8ClampedArray(this.npix * 4); this.q.enqueueReadBuffer(this.pixel, false, 0, o.length, o, []); this.q.finish(); return o; }
  readRadiance() { const o = new Float32Array(this.npix * 4); this.q.enqueueReadBuffer(this.radiance, false, 0, o.byteLength, o, []); this.q.finish(); return o; }
  readAcu() { const a = new Float32Array(this.nrays * 4); this.q.enqueueReadBuffer(this.acu, false, 0, a.byteLength, a, []); this.q.finish(); return a; }
  release() {
    [this.seeds, this.acu, this.pixel, this.radiance, this.normalHits, this.albedoDepth, this.filtered, this.filteredPixel, this.ao].forEach((b) => b && b.release());
    this.dev.bufs.forEach((b) => b.release());
    this.q.release();
    if (this.ownCtx) this.ctx.release();
  }
}

// One frame over N devices of this process: contiguous row tiles (mirt_tile_rows), global ray ids, every device runs the fused pass on
// its tile (launches are asynchronous: the one JS thread queues them all, the devices run concurrently), then the RGBA8 and radiance
// tiles are gathered on device 0 (group.gather: RCCL over xGMI for N > 1) and read back once.  The image is identical for every N.
function renderTiled(packed, nDevices, passes, opt) {
  opt = opt || {};
  const all = webcl.getPlatforms()[0].getDevices(webcl.DEVICE_TYPE_ALL);
  // rehearsal (MIRT_GROUP_ALLOW_REPEATED_DEVICES=1, include/mirt.h): more tiles than devices -- the contexts share the devices at hand
  const rehearse = process.env.MIRT_GROUP_ALLOW_REPEATED_DEVICES === "1";
  if (all.length < nDevices && !rehearse) throw new Error("renderTiled: " + nDevices + " devices asked for, " + all.length + " visible");
  if (packed.rays_per_pixel === 1 && nDevices > 1) throw new Error("one ray per pixel couples the rows through seeds[col] (A10 code.cl:429): render it on one device");
  const devs = [];
  for (let i = 0; i < nDevices; i++) devs.push(all[i % all.length]);
  const group = webcl.createDeviceGroup(devs);
  if (opt.upscaleTiled) { try { return renderUpscaledTiled(packed, opt.upscaleTiled.hi, group, passes, opt.upscaleTiled.factor, opt); } finally { group.release(); } }
  if (opt.postInTiles && opt.denoise && !opt.guides) { try { return renderTiledPost(packed, group, passes, opt); } finally { group.release(); } }   // (--guides PREFIX wants the gathered guides: the root route)
  const tiles = [];
  for (let i = 0; i < nDevices; i++) {
    const t = group.tileRows(packed.height, i);
    tiles.push(t.nrows ? new FusedRenderer(packed, Object.assign({}, opt, { ctx: group.contexts[i], row0: t.row0, nrows: t.nrows })) : null);
  }
  const live = tiles.filter((t) => t);
  const q0 = live[0].q;
  q0.timerStart();
  if (opt.passesInOneLaunch) live.forEach((t) => t.executePasses(passes, opt.bounces));   // one call per tile, then the gather
  else for (let p = 0; p < passes; p++) live.forEach((t) => t.executeRender(opt.bounces));
  const wantGuides = !!(opt.guides || opt.denoise);   // --denoise implies the guides: the filter runs on the root, on the gathered frame
  if (wantGuides) live.forEach((t) => t.renderGuides());   // every device its tile's guides, gathered like radiance
  const npix = packed.width * packed.height;
  const root = group.contexts[0];
  const frame = root.createBuffer(webcl.MEM_READ_WRITE, npix * 4), rad = root.createBuffer(webcl.MEM_READ_WRITE, npix * 16);
  const mk16 = (i) => group.contexts[i].createBuffer(webcl.MEM_READ_WRITE, 16);
  const dummy = tiles.map((t, i) => t || { pixel: mk16(i), radiance: mk16(i), normalHits: wantGuides ? mk16(i) : null, albedoDepth: wantGuides ? mk16(i) : null, npix: 0 });
  group.gather(dummy.map((t) => t.pixel), dummy.map((t) => t.npix * 4), frame, 0, opt.forceRccl);
  group.gather(dummy.map((t) => t.radiance), dummy.map((t) => t.npix * 16), rad, 0, opt.forceRccl);
  const gnh = wantGuides ? root.createBuffer(webcl.MEM_READ_WRITE, npix * 16) : null, gad = wantGuides ? root.createBuffer(webcl.MEM_READ_WRITE, npix * 16) : null;
  if (wantGuides) {
    group.gather(dummy.map((t) => t.normalHits), dummy.map((t) => t.npix * 16), gnh, 0, opt.forceRccl);
    group.gather(dummy.map((t) => t.albedoDepth), dummy.map((t) => t.npix * 16), gad, 0, opt.forceRccl);
  }
  // the filter has no tiles: it runs once, on the root, over the gathered radiance and guides (filtering the tiles separately would differ near their borders)
  const fil = opt.denoise ? root.createBuffer(webcl.MEM_READ_WRITE, npix * 16) : null, filPix = opt.denoise ? root.createBuffer(webcl.MEM_READ_WRITE, npix * 4) : null;
  if (opt.denoise) {
    group.finish();
    q0.filterFrame(Object.assign({}, opt.denoise, { width: packed.width, height: packed.height, tone: 1 / (packed.rays_per_pixel * passes),
      radiance: rad, normalHits: gnh, albedoDepth: gad, filtered: fil, pixel: filPix }));
  }
  group.finish();
  const ms = q0.timerStopMs();
  // what the gather did: the route of every tile and whether each context reads the root's device directly (mirt.h MIRT_ROUTE_*)
  const routes = group.routes(), peers = tiles.map((_, i) => group.peerAccess(0, i));
  const pixel = new Uint8ClampedArray(npix * 4), radiance = new Float32Array(npix * 4);
  q0.enqueueReadBuffer(frame, true, 0, pixel.length, pixel, []);
  q0.enqueueReadBuffer(rad, true, 0, radiance.byteLength, radiance, []);
  q0.finish();
  let guides;
  if (opt.guides) {
    guides = { normalHits: new Float32Array(npix * 4), albedoDepth: new Float32Array(npix * 4) };
    q0.enqueueReadBuffer(gnh, true, 0, npix * 16, guides.normalHits, []);
    q0.enqueueReadBuffer(gad, true, 0, npix * 16, guides.albedoDepth, []);
    q0.finish();
  }
  let denoised;
  if (opt.denoise) {
    denoised = { pixel: new Uint8ClampedArray(npix * 4), filtered: new Float32Array(npix * 4) };
    q0.enqueueReadBuffer(filPix, true, 0, npix * 4, denoised.pixel, []);
    q0.enqueueReadBuffer(fil, true, 0, npix * 16, denoised.filtered, []);
    q0.finish();
  }
  const res = { pixel: pixel, radiance: radiance, guides: guides, denoised: denoised, ms: ms, device: live.length + " x " + live[0].device.getInfo(webcl.DEVICE_NAME), tiles: tiles.map((t) => (t ? [t.row0, t.nrows] : [0, 0])), routes: routes, peerAccess: peers };
  live.forEach((t) => t.release());
  group.release();
  return res;
}

// ---- the post-process chain in row tiles (opt.postInTiles): every context filters / upsamples the rows it rendered after a halo exchange
// (group.exchangeRows, queue.filterFrameRows, queue.upsampleFrameRows; include/mirt.h), and only finished rows are gathered.  The frames are, bit
// for bit, those of the single-context chain.  Helpers of renderTiled and renderUpscaled; `bufs` collects what the caller releases.
function tileRenderers(group, packed, opt) {
  return group.contexts.map((c, i) => {
    const t = group.tileRows(packed.height, i);
    return t.nrows ? new FusedRenderer(packed, Object.assign({}, opt, { ctx: c, row0: t.row0, nrows: t.nrows })) : null;
  });
}
// the frame's passes and the tile's guides, queued on every tile's context: the route renderFile takes on one context
function renderTilesGuided(live, passes, opt) {
  live.forEach((t) => {
    if (opt.passesInOneLaunch && t.canRenderPassesGuided()) t.executePassesGuided(passes, opt.bounces);
    else if (passes === 1 && !opt.passesInOneLaunch && t.canRenderGuided()) t.executeRenderGuided(opt.bounces);
    else {
      if (opt.passesInOneLaunch) t.executePasses(passes, opt.bounces);
      else for (let p = 0; p < passes; p++) t.executeRender(opt.bounces);
      t.renderGuides();
    }
  });
}
const ownRows = (tiles) => tiles.map((t) => (t ? { row0: t.row0, nrows: t.nrows } : { row0: 0, nrows: 0 }));
// one exchange: src[i] holds the rows own[i] of context i; -> per context a buffer with the rows want[i] (null where it wants none)
function exchangeTiles(group, bufs, src, own, want, rowBytes) {
  const dst = want.map((w, i) => (w.nrows ? group.contexts[i].createBuffer(webcl.MEM_READ_WRITE, w.nrows * rowBytes) : null));
  dst.forEach((b) => b && bufs.push(b));
  group.exchangeRows(src.map((b, i) => (own[i].nrows ? b : null)), own, dst, want, rowBytes);
  return dst;
}
// three exchanges fill every tile's filter window, then the tile is filtered where it is: -> { filtered, pixel }: per context a buffer of its own rows
function filterTiles(group, bufs, tiles, packed, tone, f, wantPixel) {
  const iterations = f.iterations === undefined || f.iterations === null ? webcl.FILTER_DEFAULTS.iterations : f.iterations;
  const own = ownRows(tiles), rowBytes = packed.width * 16;
  const want = own.map((o) => (o.nrows ? webcl.filterWindowRows(packed.height, o.row0, o.nrows, iterations) : { row0: 0, nrows: 0 }));
  const win = ["radiance", "normalHits", "albedoDepth"].map((k) => exchangeTiles(group, bufs, tiles.map((t) => t && t[k]), own, want, rowBytes));
  const mk = (i, bytes) => { const b = group.contexts[i].createBuffer(webcl.MEM_READ_WRITE, bytes || 16); bufs.push(b); return b; };
  const filtered = tiles.map((t, i) => mk(i, t ? t.npix * 16 : 0)), pixel = wantPixel ? tiles.map((t, i) => mk(i, t ? t.npix * 4 : 0)) : null;
  tiles.forEach((t, i) => {
    if (t) t.q.filterFrameRows(Object.assign({}, f, { width: packed.width, height: want[i].nrows, imageHeight: packed.height, winRow0: want[i].row0, row0: t.row0, nrows: t.nrows,
      tone: tone, radiance: win[0][i], normalHits: win[1][i], albedoDepth: win[2][i], filtered: filtered[i], pixel: pixel ? pixel[i] : undefined }));
  });
  return { filtered: filtered, pixel: pixel };
}
// gathers per-context buffers (bytes[i] of each) on context 0 and reads them back into `into`
function gatherTiles(group, bufs, parts, bytes, into, opt) {
  const root = group.contexts[0], total = bytes.reduce((a, b) => a + b, 0);
  const out = root.createBuffer(webcl.MEM_READ_WRITE, total || 16);
  bufs.push(out);
  group.gather(parts, bytes, out, 0, opt.forceRccl);
  group.finish();
  const q = root.createCommandQueue();
  q.enqueueReadBuffer(out, true, 0, total, into, []);
  q.finish();
  return into;
}
// renderTiled with opt.denoise and opt.postInTiles: 4 B per pixel (20 with the filtered sums; opt.filtered === false leaves them) into the root
// instead of pixel, radiance and both guides
function renderTiledPost(packed, group, passes, opt) {
  const tiles = tileRenderers(group, packed, opt), live = tiles.filter((t) => t), bufs = [];
  try {
    const q0 = live[0].q, npix = packed.width * packed.height;
    q0.timerStart();
    renderTilesGuided(live, passes, opt);
    const out = filterTiles(group, bufs, tiles, packed, 1 / (packed.rays_per_pixel * passes), opt.denoise, true);
    group.finish();
    const ms = q0.timerStopMs();
    const denoised = { pixel: gatherTiles(group, bufs, out.pixel, tiles.map((t) => (t ? t.npix * 4 : 0)), new Uint8ClampedArray(npix * 4), opt) };
    if (opt.filtered !== false) denoised.filtered = gatherTiles(group, bufs, out.filtered, tiles.map((t) => (t ? t.npix * 16 : 0)), new Float32Array(npix * 4), opt);
    return { pixel: denoised.pixel, denoised: denoised, ms: ms, device: live.length + " x " + live[0].device.getInfo(webcl.DEVICE_NAME),
             tiles: tiles.map((t) => (t ? [t.row0, t.nrows] : [0, 0])), routes: group.routes(), peerAccess: tiles.map((_, i) => group.peerAccess(0, i)), postInTiles: true };
  } finally {
    bufs.forEach((b) => b.release());
    live.forEach((t) => t.release());
  }
}
// renderUpscaled with opt.gpus and opt.postInTiles: the LOW frame in row tiles, filtered there with opt.denoise; one exchange moves the (filtered) low
// radiance and the two low guides into every context's low window; every context renders the guides of its OUTPUT tile and rebuilds it
function renderUpscaledTiled(lo, hi, group, passes, factor, opt) {
  const tiles = tileRenderers(group, lo, opt), live = tiles.filter((t) => t), bufs = [];
  try {
    const q0 = live[0].q, npix = hi.width * hi.height, tone = 1 / (lo.rays_per_pixel * passes);
    q0.timerStart();
    renderTilesGuided(live, passes, opt);
    const radiance = opt.denoise ? filterTiles(group, bufs, tiles, lo, tone, opt.denoise, false).filtered : tiles.map((t) => t && t.radiance);
    const own = ownRows(tiles), high = group.contexts.map((_, i) => group.tileRows(hi.height, i));
    const want = high.map((h) => (h.nrows ? webcl.upsampleLowRows(hi.height, factor, h.row0, h.nrows) : { row0: 0, nrows: 0 }));
    const low = [radiance, tiles.map((t) => t && t.normalHits), tiles.map((t) => t && t.albedoDepth)].map((src) => exchangeTiles(group, bufs, src, own, want, lo.width * 16));
    const mk = (i, bytes) => { const b = group.contexts[i].createBuffer(webcl.MEM_READ_WRITE, bytes || 16); bufs.push(b); return b; };
    const up = high.map((h, i) => mk(i, h.nrows * hi.width * 16)), px = high.map((h, i) => mk(i, h.nrows * hi.width * 4));
    let scenes = [];   // a context whose low tile is empty still rebuilds its output rows: it needs the scene for their guides
    high.forEach((h, i) => {
      if (!h.nrows) return;
      let t = tiles[i];
      if (!t) { t = new FusedRenderer(lo, Object.assign({}, opt, { ctx: group.contexts[i], row0: 0, nrows: 1 })); scenes.push(t); }
      const nh = mk(i, h.nrows * hi.width * 16), ad = mk(i, h.nrows * hi.width * 16);
      t.q.renderGuides(Object.assign(t.passDesc(), { width: hi.width, height: hi.height, row0: h.row0, nrows: h.nrows, cam: hi.cam }), nh, ad);
      t.q.upsampleFrameRows(Object.assign({}, opt.upsample, { width: hi.width, height: hi.height, factor: factor, tone: tone, row0: h.row0, nrows: h.nrows,
        loRow0: want[i].row0, loNrows: want[i].nrows, radianceLo: low[0][i], normalHitsLo: low[1][i], albedoDepthLo: low[2][i], normalHits: nh, albedoDepth: ad,
        upsampled: up[i], pixel: px[i] }));
    });
    group.finish();
    const ms = q0.timerStopMs();
    const res = { pixel: gatherTiles(group, bufs, px, high.map((h) => h.nrows * hi.width * 4), new Uint8ClampedArray(npix * 4), opt),
                  upsampled: gatherTiles(group, bufs, up, high.map((h) => h.nrows * hi.width * 16), new Float32Array(npix * 4), opt), ms: ms,
                  device: live.length + " x " + live[0].device.getInfo(webcl.DEVICE_NAME), fusedPasses: 0, guidedPasses: live.reduce((a, t) => a + (t.ctx.guidedPasses ? t.ctx.guidedPasses() : 0), 0),
                  lowWidth: lo.width, lowHeight: lo.height, postInTiles: true };
    scenes.forEach((t) => t.release());
    return res;
  } finally {
    bufs.forEach((b) => b.release());
    live.forEach((t) => t.release());
  }
}

// per-pixel sequential fp32 sums of the per-ray accumulators (copyToPixel's order, A10 code.cl:1377-1380)
function radianceSums(acu, rpp) {
  const n = acu.length / 4 / rpp, out = new Float32Array(n * 4);
  for (let px = 0; px < n; px++) for (let i = 0; i < rpp; i++) for (let c = 0; c < 4; c++) out[4 * px + c] = Math.fround(out[4 * px + c] + acu[4 * (px * rpp + i) + c]);
  return out;
}

function renderFile(file, width, height, rpp, passes, opt) {
  opt = opt || {};
  let packed, ownCtx = null;
  if (opt.deviceGrid) {   // the host only reads the files: mesh ingest (node x mesh transforms, de-indexing: parseMeshJSON), binning, mesh
                          // transforms and fp32 narrowing all happen on the device
    ownCtx = webcl.createContext(pickDevice(opt.device));
    const q = ownCtx.createCommandQueue();
    const parseMesh = (model) => {
      const r = q.meshIngest(model, scene.normalFromMat4);
      r.model = model;   // a row tile on another device ingests it again there (buildSceneOnDevice)
      const b = r.bounds6.map((v) => (v === Infinity ? Number.MAX_VALUE : v === -Infinity ? -Number.MAX_VALUE : v));   // an empty mesh keeps Bounds' initial values
      r.bounds = new scene.Bounds(b.slice(0, 3), b.slice(3));
      return r;
    };
    const sc = scene.loadSceneFile(file, width, height, { deferGrids: true, parseMesh: opt.hostIngest ? undefined : parseMesh });
    packed = scene.packScene(sc, width, height, rpp, 1, true);
    opt = Object.assign({}, opt, { sceneObject: sc, ctx: ownCtx });
  } else packed = scene.packScene(scene.loadSceneFile(file, width, height), width, height, rpp);
  if (opt.ao && opt.gpus) throw new Error("--ao is not available with --gpus N: gathering the tiles' AO pairs is not built");
  if (opt.everyPass && opt.gpus > 1) throw new Error("--every-pass is not available with --gpus N > 1: the gather would interleave the tiles' frames");
  if (opt.gpus && !(opt.everyPass && opt.gpus === 1)) {
    // N contexts, one per device: each builds its own copy of the scene (the loader's soups stay on ownCtx until every tile is built)
    if (opt.sceneObject) opt.sceneObject.keepSoups = true;
    try { return renderTiled(packed, opt.gpus, passes, opt); } finally { if (ownCtx) ownCtx.release(); }
  }
  if (opt.ao && opt.granular) throw new Error("--ao is the fused host's (mirt_render_ao): not with the kernel-by-kernel host");
  if (opt.everyPass && !opt.passesInOneLaunch) throw new Error("--every-pass writes the frames of passes in one launch: give --passes-in-one-launch too");
  if ((opt.guides || opt.denoise) && opt.granular) throw new Error("--guides and --denoise are the fused host's (mirt_render_guides, mirt_filter_atrous): not with the kernel-by-kernel host");
  if (opt.passesInOneLaunch && opt.granular) throw new Error("passes in one launch are the fused pass's (mirt_render_passes): not with the kernel-by-kernel host");
  const R = opt.granular ? new GranularRenderer(packed, opt) : new FusedRenderer(packed, opt);
  // --ao: ambient occlusion of the first hit, taken before the first pass -- from the seeds the frame starts with, which it does not advance, so the
  // frame is the same with and without it
  let ao = null;
  if (opt.ao) { R.renderAo(opt.ao); ao = { pairs: R.readAo(), deferred: R.q.aoDeferred() }; }
  // one pass and its guides wanted: the pass writes them too (mirt_render_first_pass_guided), the files are the same bit for bit
  // passes in one launch and the guides wanted: that call writes them (mirt_render_passes_guided), with or without a frame after every pass
  const passesGuided = !!(opt.guides || opt.denoise) && !!opt.passesInOneLaunch && !opt.granular && R.canRenderPassesGuided();
  const guided = passesGuided || (!!(opt.guides || opt.denoise) && passes === 1 && !opt.passesInOneLaunch && R.canRenderGuided());
  R.q.timerStart();
  if (passesGuided) R.executePassesGuided(passes, opt.bounces, { everyPass: opt.everyPass });
  else if (guided) R.executeRenderGuided(opt.bounces);
  else if (opt.passesInOneLaunch) R.executePasses(passes, opt.bounces, { everyPass: opt.everyPass });
  else for (let i = 0; i < passes; i++) R.executeRender(opt.bounces);
  const ms = R.q.timerStopMs();
  const res = { pixel: R.readPixels(), radiance: opt.granular ? radianceSums(R.readAcu(), rpp) : R.readRadiance(), ms: ms,
                device: R.device.getInfo(webcl.DEVICE_NAME), fusedPasses: R.ctx.fusedPasses ? R.ctx.fusedPasses() : 0,
                guidedPasses: R.ctx.guidedPasses ? R.ctx.guidedPasses() : 0 };
  if (opt.everyPass) res.frames = R.readFrames();
  if (ao) res.ao = ao;
  if (opt.guides) { if (!guided) R.renderGuides(); res.guides = R.readGuides(); }
  if (opt.denoise) { R.denoise(opt.denoise, guided || !!opt.guides); res.denoised = R.readDenoised(); }
  R.release();
  if (ownCtx) ownCtx.release();
  return res;
}

// Shade at 1/factor resolution, output at full (queue.upsampleFrame, mirt_upsample_guided).  width x height is the OUTPUT size, rpp the rays per
// LOW pixel.  The scene file is loaded twice -- at (width / factor) x (height / factor), which the fused renderer traces, and at width x height for
// the camera pack of the full-resolution guides: the camera's window is given in scene space, so both cover the same frustum.  On the device, in
// order: the passes, the low guides, opt.denoise: the a-trous filter of the low frame, the guides at the output size, the upsampler.  One context
// and whole frames: the upsampler, like the filter, has no tiles.
function renderUpscaled(file, width, height, rpp, passes, factor, opt) {
  opt = opt || {};
  if (opt.gpus && !opt.postInTiles) throw new Error("--upscale is not available with --gpus N: the upsampler, like the filter, wants whole frames on one context, and gathering the low frame and both pairs of guides is not built");
  if (opt.gpus && opt.guides) throw new Error("--upscale with --gpus N --post-in-tiles gathers the finished rows only: not with --guides");
  if (opt.granular || opt.everyPass || opt.deviceGrid) throw new Error("--upscale drives the fused host on host-built grids: not with --granular, --every-pass or --device-grid");
  if (!(factor >= 2 && factor <= 4) || factor !== Math.floor(factor)) throw new Error(`--upscale ${factor}: the factor is 2, 3 or 4`);
  if (width % factor || height % factor) throw new Error(`--upscale ${factor}: ${width}x${height} is not a multiple of the factor (the two images would not show the same frustum)`);
  const wl = width / factor, hl = height / factor;
  const lo = scene.packScene(scene.loadSceneFile(file, wl, hl), wl, hl, rpp);
  const hi = scene.packScene(scene.loadSceneFile(file, width, height), width, height, rpp);
  if (opt.gpus) return renderTiled(lo, opt.gpus, passes, Object.assign({}, opt, { upscaleTiled: { hi: hi, factor: factor } }));   // the post chain in row tiles
  const R = new FusedRenderer(lo, opt);
  const npix = width * height;
  const mk = (bytes) => R.ctx.createBuffer(webcl.MEM_READ_WRITE, bytes);
  const nh = mk(npix * 16), ad = mk(npix * 16), up = mk(npix * 16), px = mk(npix * 4);
  try {
    R.q.timerStart();
    const passesGuided = !!opt.passesInOneLaunch && R.canRenderPassesGuided();   // the low frame's passes in one launch write the low guides too
    const guided = passesGuided || (passes === 1 && !opt.passesInOneLaunch && R.canRenderGuided());   // ... or its one pass does
    if (passesGuided) R.executePassesGuided(passes, opt.bounces);
    else if (guided) R.executeRenderGuided(opt.bounces);
    else if (opt.passesInOneLaunch) R.executePasses(passes, opt.bounces);
    else for (let i = 0; i < passes; i++) R.executeRender(opt.bounces);
    if (!guided) R.renderGuides();
    if (opt.denoise) R.denoise(opt.denoise, true);
    R.q.renderGuides(Object.assign(R.passDesc(), { width: width, height: height, row0: 0, nrows: height, cam: hi.cam }), nh, ad);
    R.q.upsampleFrame(Object.assign({}, opt.upsample, { width: width, height: height, factor: factor, tone: 1 / (rpp * (R.passes - 1)),
      radianceLo: opt.denoise ? R.filtered : R.radiance, normalHitsLo: R.normalHits, albedoDepthLo: R.albedoDepth, normalHits: nh, albedoDepth: ad,
      upsampled: up, pixel: px }));
    const ms = R.q.timerStopMs();
    const read = (b, a) => { R.q.enqueueReadBuffer(b, true, 0, a.byteLength, a, []); return a; };
    const res = { pixel: read(px, new Uint8ClampedArray(npix * 4)), upsampled: read(up, new Float32Array(npix * 4)), radiance: R.readRadiance(), ms: ms,
                  guides: { normalHits: read(nh, new Float32Array(npix * 4)), albedoDepth: read(ad, new Float32Array(npix * 4)) }, guidesLo: R.readGuides(),
                  device: R.device.getInfo(webcl.DEVICE_NAME), fusedPasses: 0, guidedPasses: R.ctx.guidedPasses ? R.ctx.guidedPasses() : 0, lowWidth: wl, lowHeight: hl };
    if (opt.denoise) res.denoised = R.readDenoised();
    R.q.finish();
    return res;
  } finally {
    [nh, ad, up, px].forEach((b) => b.release());
    R.release();
  }
}

// Ray queries on a scene file (queue.traceClosest / traceOccluded): `rays` a Float32Array of 8 floats per ray {o.xyz, mint, d.xyz, maxt}.
// opt.occluded: -> {occluded: Uint8Array}; else -> {hits: Float32Array of 8 per ray (matId as int32 bits in the 8th), sets: Uint32Array | undefined
// (opt.sets)}; both with `deferred`, the rays the exact kernel redid.  The camera and the image size play no part.
// opt.radiance = {samples, bounces, seedBase, noEmitters}: -> {radiance: Float32Array of 4 per ray, the accumulator of the pass's path from
// each ray on (queue.traceRadiance), deferred}.
function traceFile(file, rays, opt) {
  opt = opt || {};
  const n = Math.floor(rays.length / 8);
  const packed = scene.packScene(scene.loadSceneFile(file, 8, 8), 8, 8, 4);
  const ctx = webcl.createContext(pickDevice(opt.device)), q = ctx.createCommandQueue();
  const dev = uploadScene(ctx, q, packed);
  const desc = { spheres: dev.sph, triangles: dev.tri, meshes: dev.meshes };
  const mk = (bytes) => ctx.createBuffer(webcl.MEM_READ_WRITE, Math.max(bytes, 16));
  const rb = mk(n * 32);
  if (n) q.enqueueWriteBuffer(rb, false, 0, n * 32, rays.subarray(0, n * 8), []);
  const res = {};
  if (opt.radiance) {
    // path radiance (queue.traceRadiance): opt.radiance = {samples, bounces, seedBase, noEmitters}; seeds from seedFill(0, n, seedBase)
    const o = opt.radiance, sb = mk(n * 4), ab = mk(n * 16);
    if (n) q.seedFill(sb, 0, n, o.seedBase || 0);
    q.traceRadiance({ spheres: dev.sph, triangles: dev.tri, meshes: dev.meshes, lights: packed.lights, material: dev.material, bounces: o.bounces === undefined ? 5 : o.bounces },
                    { samples: o.samples === undefined ? 1 : o.samples, flags: o.noEmitters ? 2 : 0 }, rb, n, sb, ab);
    res.radiance = new Float32Array(n * 4);
    if (n) q.enqueueReadBuffer(ab, true, 0, n * 16, res.radiance, []);
    res.deferred = q.radianceDeferred();
    ctx.release();
    return res;
  }
  if (opt.occluded) {
    const ob = mk(n);
    q.traceOccluded(desc, rb, n, ob);
    res.occluded = new Uint8Array(n);
    if (n) q.enqueueReadBuffer(ob, true, 0, n, res.occluded, []);
  } else {
    const hb = mk(n * 32), sb = opt.sets ? mk(n * 4) : null;
    q.traceClosest(desc, rb, n, hb, sb);
    res.hits = new Float32Array(n * 8);
    if (n) q.enqueueReadBuffer(hb, true, 0, n * 32, res.hits, []);
    if (sb) { res.sets = new Uint32Array(n); if (n) q.enqueueReadBuffer(sb, true, 0, n * 4, res.sets, []); }
  }
  res.deferred = q.traceDeferred();
  ctx.release();
  return res;
}

// ---- panoramic, fisheye and orthographic cameras on a scene file (queue.viewRays / renderView; include/mirt.h has the definition).
// v = {model: "equirect" | "fisheye" | "ortho", eye, look, up (3 numbers each), fov (FISHEYE: the full field of view in degrees, default 180),
// orthoSize ([w, h], the ORTHOGRAPHIC window, default the scene box's extents in x and y)}.  Left out: the eye is the scene box's centre, looking
// down -z with +y up.  The basis is computed in double -- forward = normalize(look - eye), right = normalize(forward x up), up' = right x forward
// -- and narrowed once, as pyhost/mirt.py view_desc does.
const VIEW_MODELS = { ortho: 0, orthographic: 0, equirect: 1, fisheye: 2 };
function makeView(packed, width, height, rpp, v) {
  v = v || {};
  if (!(v.model in VIEW_MODELS)) throw new Error(`--view ${v.model}: equirect, fisheye or ortho`);
  const k = Math.round(Math.sqrt(rpp));
  if (k * k !== rpp || ![1, 2, 4, 8, 16].includes(k)) throw new Error(`--view: raysPerPixel ${rpp} is not 1, 4, 16, 64 or 256`);
  const b = packed.bounds, lo = [b[0], b[1], b[2]], hi = [b[4], b[5], b[6]];
  const eye = v.eye || lo.map((x, c) => (x + hi[c]) / 2);
  const look = v.look || [eye[0], eye[1], eye[2] - 1];
  const up0 = v.up || [0, 1, 0];
  const norm = (a) => { const l = Math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); return [a[0] / l, a[1] / l, a[2] / l]; };
  const cross = (a, c) => [a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]];
  const forward = norm([look[0] - eye[0], look[1] - eye[1], look[2] - eye[2]]);
  const right = norm(cross(forward, up0));
  const up = cross(right, forward);
  const size = v.orthoSize || [hi[0] - lo[0], hi[1] - lo[1]];
  const fov = v.fov === undefined ? 180 : v.fov;
  return { model: VIEW_MODELS[v.model], width: width, height: height, k: k, eye: eye, right: right, up: up, forward: forward,
           halfW: size[0] / 2, halfH: size[1] / 2, halfAngle: fov / 2 * Math.PI / 180, tMin: 0, tMax: Infinity, tone: 1 };
}
// -> {pixel: Uint8ClampedArray, radiance: Float32Array (the sums after the last pass), ms, device, deferred}: `passes` progressive frames,
// MIRT_VIEW_ACCUMULATE from the second on, tone 1 / (rpp * p).  opt.view: makeView's v; opt.bounces; opt.seeds (Int32Array) or seedFill(0, n, 0).
// opt.guides: + guides {normalHits, albedoDepth} (Float32Array, float4 per pixel) and guidedViews -- pass 1 goes through queue.renderViewGuided
// (the guides are the same for every pass), the later ones are plain.  opt.denoise ({iterations, ...}: filterFrame's parameters, webcl.FILTER_DEFAULTS
// where left out; implies the guides on the device): + denoised {pixel, filtered}, the a-trous filter run once behind the last pass with tone
// 1 / (rpp * passes); nothing leaves the device between the passes and the filter.
// opt.ao ({samples, radius, bias}): + ao {pairs: Uint32Array {open, cast} per pixel, deferred} -- queue.viewAo (mirt_view_ao) before the first
// pass, from the seeds as they stand there (it does not advance them), outside the timed span.
function renderViewFile(file, width, height, rpp, passes, opt) {
  opt = opt || {};
  const packed = scene.packScene(scene.loadSceneFile(file, width, height), width, height, 4);
  const view = makeView(packed, width, height, rpp, opt.view);
  const ctx = webcl.createContext(pickDevice(opt.device)), q = ctx.createCommandQueue();
  if (!q.hasView()) throw new Error("the loaded addon has no renderView");
  const dev = uploadScene(ctx, q, packed);
  const npix = width * height, n = npix * rpp;
  const mk = (bytes) => ctx.createBuffer(webcl.MEM_READ_WRITE, Math.max(bytes, 16));
  const sb = mk(n * 4), rb = mk(npix * 16), pb = mk(npix * 4);
  const guided = !!(opt.guides || opt.denoise);
  if (guided && !q.hasViewGuides()) throw new Error("the loaded addon has no renderViewGuided");
  const nhb = guided ? mk(npix * 16) : null, adb = guided ? mk(npix * 16) : null;
  const fb = opt.denoise ? mk(npix * 16) : null, fpb = opt.denoise ? mk(npix * 4) : null;
  if (opt.seeds) q.enqueueWriteBuffer(sb, false, 0, n * 4, opt.seeds.subarray(0, n), []);
  else q.seedFill(sb, 0, n, 0);
  const desc = { spheres: dev.sph, triangles: dev.tri, meshes: dev.meshes, lights: packed.lights, material: dev.material, bounces: opt.bounces === undefined ? 5 : opt.bounces };
  let ao = null;
  if (opt.ao) {
    if (!q.hasViewAo()) throw new Error("the loaded addon has no viewAo");
    const ab = mk(npix * 8);
    q.viewAo(desc, view, opt.ao, sb, ab);
    ao = { pairs: new Uint32Array(npix * 2), deferred: q.viewAoDeferred() };
    q.enqueueReadBuffer(ab, true, 0, npix * 8, ao.pairs, []);
  }
  q.finish();
  const t0 = process.hrtime.bigint();
  let deferred = 0;
  for (let p = 1; p <= passes; p++) {
    const vp = Object.assign({}, view, { flags: p > 1 ? 1 : 0, tone: 1 / (rpp * p) });
    if (guided && p === 1) q.renderViewGuided(desc, vp, sb, rb, pb, nhb, adb);
    else q.renderView(desc, vp, sb, rb, pb);
    if (opt.countDeferred) deferred += q.viewDeferred();
  }
  if (opt.denoise) q.filterFrame(Object.assign({}, opt.denoise, { width: width, height: height, tone: 1 / (rpp * passes), radiance: rb, normalHits: nhb, albedoDepth: adb, filtered: fb, pixel: fpb }));
  q.finish();
  const ms = Number(process.hrtime.bigint() - t0) / 1e6;
  const res = { pixel: new Uint8ClampedArray(npix * 4), radiance: new Float32Array(npix * 4), ms: ms, device: pickDevice(opt.device).getInfo(webcl.DEVICE_NAME), deferred: deferred };
  q.enqueueReadBuffer(pb, true, 0, npix * 4, res.pixel, []);
  q.enqueueReadBuffer(rb, true, 0, npix * 16, res.radiance, []);
  if (guided) res.guidedViews = q.guidedViews();
  if (ao) res.ao = ao;
  if (opt.guides) {
    res.guides = { normalHits: new Float32Array(npix * 4), albedoDepth: new Float32Array(npix * 4) };
    q.enqueueReadBuffer(nhb, true, 0, npix * 16, res.guides.normalHits, []);
    q.enqueueReadBuffer(adb, true, 0, npix * 16, res.guides.albedoDepth, []);
  }
  if (opt.denoise) {
    res.denoised = { pixel: new Uint8ClampedArray(npix * 4), filtered: new Float32Array(npix * 4) };
    q.enqueueReadBuffer(fpb, true, 0, npix * 4, res.denoised.pixel, []);
    q.enqueueReadBuffer(fb, true, 0, npix * 16, res.denoised.filtered, []);
  }
  ctx.release();
  return res;
}
// -> {pixel: Uint8ClampedArray, radiance: Float32Array (the sums after the last pass), frames, ms, device, deferred}, each holding N frames back to
// back: the frames of N cameras in one launch per pass (queue.renderViewBatch: mirt_render_view_batch), `passes` progressive calls with
// MIRT_VIEW_ACCUMULATE from the second on and tone 1 / (rpp * p).  cameras: Float32Array of 12 per frame -- eye, right, up, forward, used as
// given -- or, with opt.eyes, of 3 per frame: the eyes of cameras with the basis right = +x, up = +y, forward = -z.  opt.view: makeView's v
// (the model and what all frames share; its eye, look and up are not used); opt.bounces; opt.seedBase: seedFill(0, n, seedBase).
// opt.guides: + guides {normalHits, albedoDepth} (Float32Array, float4 per pixel, N frames back to back) and guidedViews -- pass 1 goes through
// queue.renderViewGuidedBatch (mirt_render_view_guided_batch), the later ones are plain.  opt.ao ({samples, radius, bias}): + ao {pairs:
// Uint32Array {open, cast} per pixel, deferred} -- queue.viewAoBatch (mirt_view_ao_batch) before the first pass, from the seeds as they stand
// there (it does not advance them), outside the timed span.
function renderViewBatchFile(file, cameras, width, height, rpp, passes, opt) {
  opt = opt || {};
  const per = opt.eyes ? 3 : 12;
  if (cameras.length % per) throw new Error(`cameras: ${cameras.length} floats is not a whole number of ${per} per frame`);
  const frames = cameras.length / per;
  let table = cameras;
  if (opt.eyes) {
    table = new Float32Array(frames * 12);
    for (let f = 0; f < frames; f++) table.set([cameras[3 * f], cameras[3 * f + 1], cameras[3 * f + 2], 1, 0, 0, 0, 1, 0, 0, 0, -1], 12 * f);
  }
  const packed = scene.packScene(scene.loadSceneFile(file, width, height), width, height, 4);
  const view = makeView(packed, width, height, rpp, opt.view);
  for (const name of ["eye", "right", "up", "forward"]) delete view[name];
  const ctx = webcl.createContext(pickDevice(opt.device)), q = ctx.createCommandQueue();
  if (!q.hasViewBatch()) throw new Error("the loaded addon has no renderViewBatch");
  const dev = uploadScene(ctx, q, packed);
  const npix = frames * width * height, n = npix * rpp;
  const mk = (bytes) => ctx.createBuffer(webcl.MEM_READ_WRITE, Math.max(bytes, 16));
  const sb = mk(n * 4), rb = mk(npix * 16), pb = mk(npix * 4);
  if ((opt.guides || opt.ao) && !q.hasViewBatchAov()) throw new Error("the loaded addon has no renderViewGuidedBatch / viewAoBatch");
  const nhb = opt.guides ? mk(npix * 16) : null, adb = opt.guides ? mk(npix * 16) : null;
  if (n) q.seedFill(sb, 0, n, opt.seedBase || 0);
  const desc = { spheres: dev.sph, triangles: dev.tri, meshes: dev.meshes, lights: packed.lights, material: dev.material, bounces: opt.bounces === undefined ? 5 : opt.bounces };
  let ao = null;
  if (opt.ao) {
    const ab = mk(npix * 8);
    q.viewAoBatch(desc, view, table, opt.ao, sb, ab);
    ao = { pairs: new Uint32Array(npix * 2), deferred: npix ? q.viewAoDeferred() : 0 };
    if (npix) q.enqueueReadBuffer(ab, true, 0, npix * 8, ao.pairs, []);
  }
  q.finish();
  const t0 = process.hrtime.bigint();
  let deferred = 0;
  for (let p = 1; p <= passes; p++) {
    const vp = Object.assign({}, view, { flags: p > 1 ? 1 : 0, tone: 1 / (rpp * p) });
    if (opt.guides && p === 1) q.renderViewGuidedBatch(desc, vp, table, sb, rb, pb, nhb, adb);
    else q.renderViewBatch(desc, vp, table, sb, rb, pb);
    if (opt.countDeferred) deferred += q.viewDeferred();
  }
  q.finish();
  const ms = Number(process.hrtime.bigint() - t0) / 1e6;
  const res = { pixel: new Uint8ClampedArray(npix * 4), radiance: new Float32Array(npix * 4), frames: frames, ms: ms, device: pickDevice(opt.device).getInfo(webcl.DEVICE_NAME), deferred: deferred };
  if (npix) {
    q.enqueueReadBuffer(pb, true, 0, npix * 4, res.pixel, []);
    q.enqueueReadBuffer(rb, true, 0, npix * 16, res.radiance, []);
  }
  if (ao) res.ao = ao;
  if (opt.guides) {
    res.guidedViews = q.guidedViews();
    res.guides = { normalHits: new Float32Array(npix * 4), albedoDepth: new Float32Array(npix * 4) };
    if (npix) {
      q.enqueueReadBuffer(nhb, true, 0, npix * 16, res.guides.normalHits, []);
      q.enqueueReadBuffer(adb, true, 0, npix * 16, res.guides.albedoDepth, []);
    }
  }
  ctx.release();
  return res;
}
// -> Float32Array of 8 per ray: the view's rays themselves (queue.viewRays), for callers who want them
function viewRaysFile(file, width, height, rpp, opt) {
  opt = opt || {};
  const packed = scene.packScene(scene.loadSceneFile(file, width, height), width, height, 4);
  const view = makeView(packed, width, height, rpp, opt.view);
  const ctx = webcl.createContext(pickDevice(opt.device)), q = ctx.createCommandQueue();
  const n = width * height * rpp;
  const rb = ctx.createBuffer(webcl.MEM_READ_WRITE, Math.max(n * 32, 16));
  q.viewRays(view, rb);
  const rays = new Float32Array(n * 8);
  q.enqueueReadBuffer(rb, true, 0, n * 32, rays, []);
  ctx.release();
  return rays;
}
// -> {normalHits, albedoDepth}: Float32Array of 4 per pixel each, the view's first-hit guides alone (queue.viewGuides: mirt_view_guides), no
// frame.  opt.view: makeView's v; opt.normalHits === false or opt.albedoDepth === false leaves that output out of the call (null in the result)
function viewGuidesFile(file, width, height, rpp, opt) {
  opt = opt || {};
  const packed = scene.packScene(scene.loadSceneFile(file, width, height), width, height, 4);
  const view = makeView(packed, width, height, rpp, opt.view);
  const ctx = webcl.createContext(pickDevice(opt.device)), q = ctx.createCommandQueue();
  if (!q.hasViewGuides()) throw new Error("the loaded addon has no viewGuides");
  const dev = uploadScene(ctx, q, packed);
  const npix = width * height;
  const mk = (wanted) => (wanted === false ? null : ctx.createBuffer(webcl.MEM_READ_WRITE, Math.max(npix * 16, 16)));
  const nhb = mk(opt.normalHits), adb = mk(opt.albedoDepth);
  q.viewGuides({ spheres: dev.sph, triangles: dev.tri, meshes: dev.meshes, material: dev.material }, view, nhb, adb);
  const read = (b) => { if (!b) return null; const a = new Float32Array(npix * 4); q.enqueueReadBuffer(b, true, 0, npix * 16, a, []); return a; };
  const res = { normalHits: read(nhb), albedoDepth: read(adb) };
  ctx.release();
  return res;
}

// -> {normalHits, albedoDepth, frames}: the first-hit guides alone of N cameras' frames, back to back, in one launch (queue.viewGuidesBatch:
// mirt_view_guides_batch).  cameras: Float32Array of 12 per frame, as for renderViewBatchFile; opt.view: makeView's v (what all frames share);
// opt.normalHits === false or opt.albedoDepth === false leaves that output out of the call (null in the result)
function viewGuidesBatchFile(file, cameras, width, height, rpp, opt) {
  opt = opt || {};
  if (cameras.length % 12) throw new Error(`cameras: ${cameras.length} floats is not a whole number of 12 per frame`);
  const frames = cameras.length / 12;
  const packed = scene.packScene(scene.loadSceneFile(file, width, height), width, height, 4);
  const view = makeView(packed, width, height, rpp, opt.view);
  for (const name of ["eye", "right", "up", "forward"]) delete view[name];
  const ctx = webcl.createContext(pickDevice(opt.device)), q = ctx.createCommandQueue();
  if (!q.hasViewBatchAov()) throw new Error("the loaded addon has no viewGuidesBatch");
  const dev = uploadScene(ctx, q, packed);
  const npix = frames * width * height;
  const mk = (wanted) => (wanted === false ? null : ctx.createBuffer(webcl.MEM_READ_WRITE, Math.max(npix * 16, 16)));
  const nhb = mk(opt.normalHits), adb = mk(opt.albedoDepth);
  q.viewGuidesBatch({ spheres: dev.sph, triangles: dev.tri, meshes: dev.meshes, material: dev.material }, view, cameras, nhb, adb);
  const read = (b) => { if (!b) return null; const a = new Float32Array(npix * 4); if (npix) q.enqueueReadBuffer(b, true, 0, npix * 16, a, []); return a; };
  const res = { normalHits: read(nhb), albedoDepth: read(adb), frames: frames };
  ctx.release();
  return res;
}

module.exports = { GranularRenderer, FusedRenderer, renderFile, renderUpscaled, traceFile, renderViewFile, renderViewBatchFile, viewRaysFile, viewGuidesFile, viewGuidesBatchFile, makeView, renderTiled, radianceSums, getLocalWS, KERNELS, setWebCL };
