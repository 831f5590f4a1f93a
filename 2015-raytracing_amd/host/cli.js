#!/usr/bin/env node
// host/cli.js -- command-line front end of the JavaScript host.
//   node cli.js pack   <scene.xml> <width> <height> <raysPerPixel>                 -> packed kernel inputs as JSON (stdout)
//   node cli.js render <scene.xml> <width> <height> <raysPerPixel> <passes> <out.rgba> [--granular [--graph|--fusion]] [--device-grid] [--no-acu] [--passes-in-one-launch [--every-pass]] [--bounces N] [--seeds file.i32] [--gpus N [--force-rccl] [--post-in-tiles]] [--guides PREFIX] [--denoise [iterations]] [--upscale F] [--ao PREFIX [--ao-samples N] [--ao-radius R] [--ao-bias B]]
//                                                                                   -> RGBA8 frame, or a PPM when <out> ends in .ppm (+ <out>.radiance.f32) via the N-API addon; --guides: + PREFIX.normal_hits.f32, PREFIX.albedo_depth.f32 (first-hit guide buffers, raw float4 rows); --ao: + PREFIX.ao.u32 (ambient occlusion of the first hit, mirt_render_ao: raw uint32 pairs {open, cast} per pixel, N AO rays of length R per hit sample, default 4 and unbounded, displaced by B = 0.001 along the normal; taken before the first pass, the seeds are not advanced) and PREFIX.ao.pgm (a byte per pixel, floor(255 * open / cast + 0.5), 255 where cast is 0), not with --gpus N; --denoise: <out> is the a-trous-filtered frame (mirt_filter_atrous, guided by those buffers; + <out>.filtered.f32), <out>.radiance.f32 stays the unfiltered sums; --upscale F (2..4): width x height is the OUTPUT size and raysPerPixel is per pixel of the (width / F) x (height / F) frame that is traced -- <out> is that frame rebuilt at full resolution from the guides of both sizes (mirt_upsample_guided; + <out>.upsampled.f32), <out>.radiance.f32 (and with --denoise <out>.filtered.f32) are the LOW frame, --guides PREFIX writes the full-resolution guides and PREFIX.normal_hits_lo.f32 / .albedo_depth_lo.f32; not with --gpus N unless --post-in-tiles; --post-in-tiles (with --gpus N): --denoise and --upscale run tile-local -- every device exchanges halo rows with its neighbours and filters / upsamples its own rows (mirt_exchange_rows, mirt_filter_atrous_rows, mirt_upsample_guided_rows), only finished rows are gathered; the same bytes in <out>, <out>.filtered.f32 and <out>.upsampled.f32, and no <out>.radiance.f32 (the unfiltered sums stay on their devices)
//   node cli.js render <scene.xml> <width> <height> <raysPerPixel> <passes> <out.ppm> --view equirect|fisheye|ortho [--eye x,y,z] [--look x,y,z] [--up x,y,z] [--fov degrees] [--ortho-size w,h] [--bounces N] [--seeds file.i32] [--view-guides PREFIX] [--view-denoise [iterations]] [--view-ao PREFIX [--ao-samples N] [--ao-radius R] [--ao-bias B]]  -> a frame of a panoramic (360 x 180 degrees), fisheye (equidistant, --fov the full field of view, default 180) or orthographic (--ortho-size the window, default the scene box's extents in x and y) camera, one launch per pass (mirt_render_view): raysPerPixel 1, 4, 16, 64 or 256, un-jittered; the default eye is the scene box's centre, looking down -z; passes are progressive (MIRT_VIEW_ACCUMULATE, tone 1 / (raysPerPixel * p)); + <out>.radiance.f32; --view-guides: + PREFIX.normal_hits.f32, PREFIX.albedo_depth.f32, the camera's first-hit guides (mirt_view_guides' definition; taken by the first pass, mirt_render_view_guided); --view-denoise: <out> is the a-trous-filtered frame (mirt_filter_atrous behind the last pass, on the device; + <out>.filtered.f32), <out>.radiance.f32 stays the unfiltered sums; --view-ao: + PREFIX.ao.u32 (the camera's ambient occlusion, mirt_view_ao: raw uint32 pairs {open, cast} per pixel, N, R and B as for --ao; taken before the first pass, the seeds are not advanced) and PREFIX.ao.pgm (a byte per pixel, floor(255 * open / cast + 0.5), 0 where cast is 0); not with --gpus, --guides, --denoise, --ao (the thin-lens camera's), --upscale
//   node cli.js views <scene.xml> cameras.f32 <width> <height> <raysPerPixel> <passes> out.radiance.f32 --view equirect|fisheye|ortho [--eyes] [--bounces N] [--seed-base X] [--ppm PREFIX] [--guides PREFIX] [--ao PREFIX [--ao-samples N] [--ao-radius R] [--ao-bias B]] [camera options shared by all frames]  -> the frames of N cameras in one launch per pass (mirt_render_view_batch): cameras.f32 holds 12 raw floats per frame -- eye, right, up, forward, used as given -- or, with --eyes, 3 per frame: the eyes of cameras with right = +x, up = +y, forward = -z; out.radiance.f32 receives the N frames of float4 sums back to back; --ppm PREFIX: + PREFIX.<frame>.ppm, one picture per frame; --guides PREFIX: + PREFIX.normal_hits.f32 and PREFIX.albedo_depth.f32, the N frames' first-hit guides back to back (taken by the first pass, mirt_render_view_guided_batch); --ao PREFIX: + PREFIX.ao.u32, the N frames' ambient occlusion back to back (mirt_view_ao_batch: raw uint32 pairs {open, cast} per pixel, N, R and B as for render's --ao; taken before the first pass, the seeds are not advanced); the camera options that all frames share are --fov and --ortho-size; seeds from mirt_seed_fill(first_ray = 0, count, X)
//   node cli.js pack-frame <1|4|7> <mesh.json|mol.pdb|-> <width> <height> [nSlabs]  -> packed inputs of an Assign01/04/07 frame job (stdout)
//   node cli.js frame      <1|4|7> <mesh.json|mol.pdb|-> [<mol.pdb>] <width> <height> <nSlabs|0> <out.rgba> [--one-launch] [--aa K]  -> RGBA8 frame of that job; 7 with a mesh AND a molecule: both models (computeBoth); --one-launch: the whole frame in one launch, no ray buffer; --aa K (1 to 4, not with 1): K x K samples a pixel averaged in that one launch
//   node cli.js ingest <mesh.json> <out-prefix> [--device]                          -> parseMeshJSON's arrays (<out>.pos.f64, .nor.f64, .meta.json) by the host or the device
//   node cli.js trace  <scene.xml> <rays.f32> <out.f32> [--occluded] [--sets out.u32]  -> ray queries on the caller's own rays (mirt_trace_closest): rays.f32 holds raw 32-byte records {o.xyz, mint, d.xyz, maxt}, out.f32 receives {normal.xyz, t, p.xyz, matId (int32)} per ray, --sets the uint32 index of the winning set per ray; --occluded: <out.f32> receives one byte per ray instead, 1 iff something blocks it (mirt_trace_occluded)
//   node cli.js trace  <scene.xml> <rays.f32> <out.f32> --radiance [--samples S] [--bounces B] [--seed-base X] [--no-emitters]  -> path radiance of the caller's own rays in one launch (mirt_trace_radiance): out.f32 receives 16 bytes per ray, the accumulator {r, g, b sums, number of contributions} of S (default 1) runs of the pass's path with B (default 5) bounces from each ray on; seeds from mirt_seed_fill(first_ray = 0, count, X); --no-emitters: the lights are not rendered on the caller's ray (it continues a path whose vertex already sampled them)
//   node cli.js trace  <scene.xml> <W>x<H>x<raysPerPixel> <rays-out.f32> --view-rays --view equirect|fisheye|ortho [camera options as above]  -> the camera's rays themselves (mirt_view_rays): raw 32-byte records in (pixel, sy, sx) order, ready for the queries above
//   node cli.js devices                                                             -> what webcl.getPlatforms()/getDevices() report
"use strict";
const fs = require("fs");
const path = require("path");
const scene = require("./scene.js");

// <out> ending in .ppm: a binary PPM (P6) any viewer opens; anything else: the raw RGBA8 frame the page would have put on its canvas
function writeFrame(out, px, w, h) {
  const rgba = Buffer.from(px.buffer, px.byteOffset, px.byteLength);
  if (!/\.ppm$/i.test(out)) { fs.writeFileSync(out, rgba); return; }
  const rgb = Buffer.alloc(w * h * 3);
  for (let i = 0, j = 0; i < w * h * 4; i += 4, j += 3) { rgb[j] = rgba[i]; rgb[j + 1] = rgba[i + 1]; rgb[j + 2] = rgba[i + 2]; }
  fs.writeFileSync(out, Buffer.concat([Buffer.from(`P6\n${w} ${h}\n255\n`, "ascii"), rgb]));
}

// the camera options of --view (render) and --view-rays (trace): -> renderer.makeView's v
function viewOptions(rest) {
  const vi = rest.indexOf("--view");
  if (vi < 0 || !rest[vi + 1]) usage();
  const v = { model: rest[vi + 1] };
  if (!["equirect", "fisheye", "ortho"].includes(v.model)) { process.stderr.write(`--view ${v.model}: equirect, fisheye or ortho\n`); process.exit(2); }
  const list = (flag, n) => {
    const i = rest.indexOf(flag);
    if (i < 0) return undefined;
    const a = String(rest[i + 1] || "").split(",").map(Number);
    if (a.length !== n || a.some((x) => !Number.isFinite(x))) { process.stderr.write(`${flag} takes ${n} numbers separated by commas\n`); process.exit(2); }
    return a;
  };
  v.eye = list("--eye", 3); v.look = list("--look", 3); v.up = list("--up", 3); v.orthoSize = list("--ortho-size", 2);
  const f = list("--fov", 1);
  if (f) v.fov = f[0];
  return v;
}

function usage() {
  process.stderr.write(fs.readFileSync(__filename, "utf8").split("\n").slice(1, 16).join("\n") + "\n");
  process.exit(2);
}

const [cmd, ...rest] = process.argv.slice(2);
if (cmd === "pack") {
  if (rest.length < 4) usage();
  const [file, w, h, rpp] = [rest[0], +rest[1], +rest[2], +rest[3]];
  const sc = scene.loadSceneFile(file, w, h);
  const p = scene.packedToJSON(scene.packScene(sc, w, h, rpp));
  p.scene = path.basename(file);
  process.stdout.write(JSON.stringify(p));
} else if (cmd === "render") {
  if (rest.length < 6) usage();
  const renderer = require("./renderer.js");
  if (rest.includes("--view")) {   // a panoramic, fisheye or orthographic camera: one launch per pass (mirt_render_view)
    // --guides, --denoise and --ao name the thin-lens camera's routes and stay refused beside --view, as they were; these cameras' own are
    // --view-guides, --view-denoise and --view-ao
    for (const flag of ["--gpus", "--guides", "--denoise", "--upscale", "--ao"])
      if (rest.includes(flag)) { process.stderr.write(`--view is not available with ${flag}: these cameras' guides, filter and AO are --view-guides PREFIX, --view-denoise [iterations] and --view-ao PREFIX; the upsampler and row tiles over N devices are not built for them\n`); process.exit(2); }
    const vopt = { view: viewOptions(rest), bounces: 5, seeds: null, countDeferred: true };
    let j;
    if ((j = rest.indexOf("--view-guides")) >= 0) { if (!rest[j + 1]) usage(); vopt.guides = rest[j + 1]; }   // the camera's first-hit guides beside the frame
    if ((j = rest.indexOf("--view-denoise")) >= 0) {   // the frame filtered on the device behind the last pass (mirt_filter_atrous); implies the guides
      vopt.denoise = {};
      if (/^\d+$/.test(rest[j + 1] || "")) vopt.denoise.iterations = +rest[j + 1];
    }
    let aoPrefix = null;
    if ((j = rest.indexOf("--view-ao")) >= 0) {   // the camera's ambient occlusion beside the frame (mirt_view_ao), before the first pass
      if (!rest[j + 1]) usage();
      aoPrefix = rest[j + 1];
      vopt.ao = {};
      if ((j = rest.indexOf("--ao-samples")) >= 0) vopt.ao.samples = +rest[j + 1];
      if ((j = rest.indexOf("--ao-radius")) >= 0) vopt.ao.radius = +rest[j + 1];
      if ((j = rest.indexOf("--ao-bias")) >= 0) vopt.ao.bias = +rest[j + 1];
    }
    if ((j = rest.indexOf("--bounces")) >= 0) vopt.bounces = +rest[j + 1];
    if ((j = rest.indexOf("--seeds")) >= 0) { const b = fs.readFileSync(rest[j + 1]); vopt.seeds = new Int32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length)); }
    const [vf, vw, vh, vrpp, vpasses, vout] = [rest[0], +rest[1], +rest[2], +rest[3], +rest[4], rest[5]];
    let res;
    try { res = renderer.renderViewFile(vf, vw, vh, vrpp, vpasses, vopt); } catch (e) { process.stderr.write(e.message + "\n"); process.exit(2); }
    const vdump = (name, a) => fs.writeFileSync(name, Buffer.from(a.buffer, a.byteOffset, a.byteLength));
    writeFrame(vout, res.denoised ? res.denoised.pixel : res.pixel, vw, vh);
    vdump(vout + ".radiance.f32", res.radiance);
    if (res.denoised) vdump(vout + ".filtered.f32", res.denoised.filtered);
    if (res.guides) { vdump(`${vopt.guides}.normal_hits.f32`, res.guides.normalHits); vdump(`${vopt.guides}.albedo_depth.f32`, res.guides.albedoDepth); }
    process.stderr.write(`rendered ${vf} ${vw}x${vh} rpp ${vrpp}, ${vpasses} pass(es), ${vopt.view.model} camera${res.denoised ? ", filtered" : ""}: ${res.ms.toFixed(2)} ms on ${res.device}; rays redone by the exact kernel: ${res.deferred}\n`);
    if (res.guidedViews !== undefined) process.stderr.write(`frames that wrote their guides: ${res.guidedViews}\n`);
    if (res.ao) {
      const a = res.ao.pairs, gray = Buffer.alloc(vw * vh);
      for (let k = 0; k < vw * vh; k++) gray[k] = a[2 * k + 1] ? Math.floor(255 * a[2 * k] / a[2 * k + 1] + 0.5) : 0;
      vdump(`${aoPrefix}.ao.u32`, a);
      fs.writeFileSync(`${aoPrefix}.ao.pgm`, Buffer.concat([Buffer.from(`P5\n${vw} ${vh}\n255\n`, "ascii"), gray]));
      process.stderr.write(`ambient occlusion: ${aoPrefix}.ao.u32, ${aoPrefix}.ao.pgm; pixels re-run in the exact kernel: ${res.ao.deferred}\n`);
    }
    process.exit(0);
  }
  if (rest.includes("--view-ao")) { process.stderr.write("--view-ao needs --view equirect|fisheye|ortho: the thin-lens camera's AO is --ao PREFIX\n"); process.exit(2); }
  const opt = { granular: rest.includes("--granular"), graph: rest.includes("--graph"), fusion: rest.includes("--fusion"), deviceGrid: rest.includes("--device-grid"), bounces: 5, seeds: null,
                keepAcu: !rest.includes("--no-acu"),   // --no-acu: a frame without the 16 bytes per ray: the pass resolves its own pixels (mirt.h; raysPerPixel
                                                        // dividing 256 or above 256) -- one pass, or
                passesInOneLaunch: rest.includes("--passes-in-one-launch"),   // all of them in one call (mirt_render_passes; with --gpus, one per tile):
                                                                               // at most 64 without the accumulator, calls of 64 with it
                everyPass: rest.includes("--every-pass") };   // ... and the frame after every pass k = 1..passes: <stem>.pass<k><ext> (+ .radiance.f32)
  let i;
  if ((i = rest.indexOf("--bounces")) >= 0) opt.bounces = +rest[i + 1];
  if ((i = rest.indexOf("--gpus")) >= 0) { opt.gpus = +rest[i + 1]; opt.forceRccl = rest.includes("--force-rccl"); }   // row tiles over N devices + gather
  opt.postInTiles = rest.includes("--post-in-tiles") && !!opt.gpus;   // with --gpus N: --denoise and --upscale filter / upsample every tile where it is, after a halo exchange
  if ((i = rest.indexOf("--guides")) >= 0) { if (!rest[i + 1]) usage(); opt.guides = rest[i + 1]; }   // first-hit guide buffers beside the frame (mirt_render_guides)
  if ((i = rest.indexOf("--ao")) >= 0) {   // ambient occlusion of the first hit beside the frame (mirt_render_ao)
    if (!rest[i + 1]) usage();
    opt.aoPrefix = rest[i + 1];
    opt.ao = {};
    let j;
    if ((j = rest.indexOf("--ao-samples")) >= 0) opt.ao.samples = +rest[j + 1];
    if ((j = rest.indexOf("--ao-radius")) >= 0) opt.ao.radius = +rest[j + 1];
    if ((j = rest.indexOf("--ao-bias")) >= 0) opt.ao.bias = +rest[j + 1];
    if (opt.gpus) { process.stderr.write("--ao is not available with --gpus N: gathering the tiles' AO pairs is not built\n"); process.exit(2); }
    if (rest.includes("--upscale") || opt.granular) { process.stderr.write("--ao goes with the fused host's plain frame: not with --upscale or --granular\n"); process.exit(2); }
  }
  if ((i = rest.indexOf("--denoise")) >= 0) {   // the frame filtered on the device (mirt_filter_atrous); implies the guides; with --gpus N: gathered, then filtered on the root
    opt.denoise = {};
    if (/^\d+$/.test(rest[i + 1] || "")) opt.denoise.iterations = +rest[i + 1];
  }
  if ((i = rest.indexOf("--seeds")) >= 0) { const b = fs.readFileSync(rest[i + 1]); opt.seeds = new Int32Array(b.buffer, b.byteOffset, b.length / 4); }
  const [file, w, h, rpp, passes, out] = [rest[0], +rest[1], +rest[2], +rest[3], +rest[4], rest[5]];
  let upscale = 0;
  if ((i = rest.indexOf("--upscale")) >= 0) {   // shade at 1/F resolution, output at full (mirt_upsample_guided); one context: the upsampler has no tiles
    if (!/^\d+$/.test(rest[i + 1] || "")) usage();
    upscale = +rest[i + 1];
    if (opt.gpus && !opt.postInTiles) { process.stderr.write("--upscale is not available with --gpus N: the upsampler, like the filter, wants whole frames on one context, and gathering the low frame and both pairs of guides is not built\n"); process.exit(2); }
  }
  if (upscale) {
    const res = renderer.renderUpscaled(file, w, h, rpp, passes, upscale, opt);
    const dump = (f, a) => fs.writeFileSync(f, Buffer.from(a.buffer, a.byteOffset, a.byteLength));
    writeFrame(out, res.pixel, w, h);
    dump(out + ".upsampled.f32", res.upsampled);
    if (res.radiance) dump(out + ".radiance.f32", res.radiance);
    if (res.denoised) dump(out + ".filtered.f32", res.denoised.filtered);
    if (opt.guides) {
      dump(`${opt.guides}.normal_hits.f32`, res.guides.normalHits);
      dump(`${opt.guides}.albedo_depth.f32`, res.guides.albedoDepth);
      dump(`${opt.guides}.normal_hits_lo.f32`, res.guidesLo.normalHits);
      dump(`${opt.guides}.albedo_depth_lo.f32`, res.guidesLo.albedoDepth);
    }
    process.stderr.write(`rendered ${file} ${res.lowWidth}x${res.lowHeight} rpp ${rpp}, ${passes} pass(es)${opt.denoise ? ", filtered" : ""}, upsampled x${upscale} to ${w}x${h}: ${res.ms.toFixed(2)} ms on ${res.device}\n`);
    process.stderr.write(`first passes that wrote their guides: ${res.guidedPasses || 0}\n`);
    process.exit(0);
  }
  const res = renderer.renderFile(file, w, h, rpp, passes, opt);
  writeFrame(out, res.denoised ? res.denoised.pixel : res.pixel, w, h);
  if (res.denoised) fs.writeFileSync(out + ".filtered.f32", Buffer.from(res.denoised.filtered.buffer, res.denoised.filtered.byteOffset, res.denoised.filtered.byteLength));
  if (res.radiance) fs.writeFileSync(out + ".radiance.f32", Buffer.from(res.radiance.buffer, res.radiance.byteOffset, res.radiance.byteLength));   // (none from --post-in-tiles: the sums are not gathered)
  if (res.guides) {
    for (const [name, a] of [["normal_hits", res.guides.normalHits], ["albedo_depth", res.guides.albedoDepth]])
      fs.writeFileSync(`${opt.guides}.${name}.f32`, Buffer.from(a.buffer, a.byteOffset, a.byteLength));
  }
  if (res.ao) {
    const a = res.ao.pairs, gray = Buffer.alloc(w * h);
    for (let k = 0; k < w * h; k++) gray[k] = a[2 * k + 1] ? Math.floor(255 * a[2 * k] / a[2 * k + 1] + 0.5) : 255;
    fs.writeFileSync(`${opt.aoPrefix}.ao.u32`, Buffer.from(a.buffer, a.byteOffset, a.byteLength));
    fs.writeFileSync(`${opt.aoPrefix}.ao.pgm`, Buffer.concat([Buffer.from(`P5\n${w} ${h}\n255\n`, "ascii"), gray]));
    process.stderr.write(`ambient occlusion: ${opt.aoPrefix}.ao.u32, ${opt.aoPrefix}.ao.pgm; pixels re-run in the exact kernel: ${res.ao.deferred}\n`);
  }
  if (res.frames) {
    const ext = path.extname(out), stem = out.slice(0, out.length - ext.length), n = w * h * 4;
    for (let k = 1; k <= res.frames.n; k++) {
      const f = `${stem}.pass${k}${ext}`, rad = res.frames.radiance.subarray((k - 1) * n, k * n);
      writeFrame(f, res.frames.pixel.subarray((k - 1) * n, k * n), w, h);
      fs.writeFileSync(f + ".radiance.f32", Buffer.from(rad.buffer, rad.byteOffset, rad.byteLength));
    }
  }
  process.stderr.write(`rendered ${file} ${w}x${h} rpp ${rpp}, ${passes} pass(es), ${opt.granular ? (opt.fusion ? "kernel-by-kernel, passes fused by the runtime" : "kernel-by-kernel") : "fused"}: ${res.ms.toFixed(2)} ms on ${res.device}; passes the runtime fused from enqueues: ${res.fusedPasses}\n`);
  if (res.postInTiles) process.stderr.write("post-process in row tiles: halo rows exchanged, finished rows gathered\n");
  process.stderr.write(`first passes that wrote their guides: ${res.guidedPasses || 0}\n`);   // calls, of one pass or of several, whose own launch wrote the guides (ctx.guidedPasses(): mirt_render_first_pass_guided and mirt_render_passes_guided); the line keeps the wording it had when only first passes counted, for whoever parses it
  if (res.routes) process.stderr.write(`gather routes per tile: ${res.routes.join(" ")}; peer access root<-tile: ${res.peerAccess.join(" ")}\n`);
} else if (cmd === "pack-frame" || cmd === "frame") {
  if (rest.length < 4) usage();
  const frame = require("./frame.js");
  const ai = rest.indexOf("--aa"), aa = ai >= 0 ? +rest[ai + 1] : undefined;   // --aa K implies one launch
  if (ai >= 0 && !(Number.isInteger(aa) && aa >= 1)) { console.error("--aa takes the number of samples per axis, 1 to 4"); process.exit(2); }
  if (ai >= 0 && +rest[0] === 1) { console.error("--aa: Assign01 has no anti-aliased frame (frame 4 and frame 7 do)"); process.exit(2); }
  const oneLaunch = rest.includes("--one-launch") || ai >= 0;
  const a = rest.filter((x, i) => x !== "--one-launch" && i !== ai && (ai < 0 || i !== ai + 1));
  const read = (f) => fs.readFileSync(f, "utf8").replace(/^\ufeff/, "");
  const assign = +a[0], text = a[1] === "-" ? null : read(a[1]);
  let model = text === null ? null : /\.pdb$/i.test(a[1]) ? { pdb: text } : JSON.parse(text);   // .pdb: Assign07's molecule mode
  if (assign === 7 && model && !model.pdb && /\.pdb$/i.test(a[2] || "")) { model = { mesh: model, pdb: read(a[2]) }; a.splice(2, 1); }   // both models
  const p = frame.packFrame(assign, model, +a[2], +a[3], +a[4] || 2);
  if (cmd === "pack-frame") { const j = scene.packedToJSON(p); if (p.mol) j.mol = scene.packedToJSON(p.mol); process.stdout.write(JSON.stringify(j)); }
  else {
    const px = frame.renderFrame(p, { oneLaunch: oneLaunch, aa: aa });
    writeFrame(a[5], px, +a[2], +a[3]);
    process.stderr.write(`frame ${assign} ${+a[2]}x${+a[3]}: ${oneLaunch ? "one launch" : "kernel by kernel"}${aa !== undefined ? `, aa ${aa} (${aa * aa} samples a pixel)` : ""}; frames the runtime fused from enqueues: ${px.fusedFrames}\n`);
  }
} else if (cmd === "ingest") {
  if (rest.length < 2) usage();
  const model = JSON.parse(fs.readFileSync(rest[0], "utf8").replace(/^\ufeff/, ""));
  let pos, nor, meta;
  if (rest.includes("--device")) {
    const { webcl } = require("./webcl.js");
    const ctx = webcl.createContext(webcl.getPlatforms()[0].getDevices(webcl.DEVICE_TYPE_ALL)[0]), q = ctx.createCommandQueue();
    const r = q.meshIngest(model, scene.normalFromMat4);
    pos = new Float64Array(r.nTriangles * 9); nor = new Float64Array(r.nTriangles * 9);
    if (r.nTriangles) { q.enqueueReadBuffer(r.positionsBuf, true, 0, pos.byteLength, pos, []); q.enqueueReadBuffer(r.normalsBuf, true, 0, nor.byteLength, nor, []); }
    meta = { nTriangles: r.nTriangles, bounds: r.bounds6, materialIndices: r.materialIndices, materials: r.materials };
    ctx.release();
  } else {
    const r = scene.parseMeshJSON(model);
    pos = new Float64Array(r.positions); nor = new Float64Array(r.normals);
    meta = { nTriangles: r.nTriangles, bounds: r.bounds.min.concat(r.bounds.max), materialIndices: r.materialIndices, materials: r.materials };
  }
  fs.writeFileSync(rest[1] + ".pos.f64", Buffer.from(pos.buffer));
  fs.writeFileSync(rest[1] + ".nor.f64", Buffer.from(nor.buffer));
  fs.writeFileSync(rest[1] + ".meta.json", JSON.stringify(meta));
} else if (cmd === "trace") {
  if (rest.length < 3) usage();
  const renderer = require("./renderer.js");
  const si = rest.indexOf("--sets");
  if (si >= 0 && !rest[si + 1]) usage();
  if (rest.includes("--view-rays")) {   // the rays of a panoramic, fisheye or orthographic camera (mirt_view_rays): <W>x<H>x<raysPerPixel> in place of the ray file
    const m = /^(\d+)x(\d+)x(\d+)$/.exec(rest[1]);
    if (!m) { process.stderr.write("--view-rays: the second argument is <W>x<H>x<raysPerPixel>\n"); process.exit(2); }
    let rays;
    try { rays = renderer.viewRaysFile(rest[0], +m[1], +m[2], +m[3], { view: viewOptions(rest) }); } catch (e) { process.stderr.write(e.message + "\n"); process.exit(2); }
    fs.writeFileSync(rest[2], Buffer.from(rays.buffer, rays.byteOffset, rays.byteLength));
    process.stderr.write(`wrote ${rays.length / 8} rays of the ${rest[rest.indexOf("--view") + 1]} camera of ${rest[0]} at ${rest[1]} to ${rest[2]}\n`);
    process.exit(0);
  }
  const raw = fs.readFileSync(rest[1]);
  if (raw.length % 32) { process.stderr.write(`${rest[1]}: ${raw.length} bytes is not a whole number of 32-byte rays\n`); process.exit(2); }
  const rays = new Float32Array(raw.length / 4);
  Buffer.from(rays.buffer).set(raw);   // (a file's bytes need not sit 4-byte aligned in node's pool)
  if (rest.includes("--radiance")) {
    if (si >= 0 || rest.includes("--occluded")) { process.stderr.write("--radiance goes without --sets and --occluded\n"); process.exit(2); }
    const num = (flag, dflt) => { const i = rest.indexOf(flag); if (i < 0) return dflt; const v = Number(rest[i + 1]); if (!Number.isInteger(v) || v < 0) usage(); return v; };
    const res = renderer.traceFile(rest[0], rays, { radiance: { samples: num("--samples", 1), bounces: num("--bounces", 5), seedBase: num("--seed-base", 0), noEmitters: rest.includes("--no-emitters") } });
    fs.writeFileSync(rest[2], Buffer.from(res.radiance.buffer, res.radiance.byteOffset, res.radiance.byteLength));
    process.stderr.write(`traced ${rays.length / 8} rays of ${rest[1]} through ${rest[0]}: path radiance; rays redone by the exact kernel: ${res.deferred}\n`);
    process.exit(0);
  }
  const occluded = rest.includes("--occluded");
  if (occluded && si >= 0) { process.stderr.write("--sets goes with the closest-hit query, not with --occluded\n"); process.exit(2); }
  const res = renderer.traceFile(rest[0], rays, { occluded: occluded, sets: si >= 0 });
  const out = occluded ? res.occluded : res.hits;
  fs.writeFileSync(rest[2], Buffer.from(out.buffer, out.byteOffset, out.byteLength));
  if (res.sets) fs.writeFileSync(rest[si + 1], Buffer.from(res.sets.buffer, res.sets.byteOffset, res.sets.byteLength));
  process.stderr.write(`traced ${rays.length / 8} rays of ${rest[1]} through ${rest[0]}: ${occluded ? "occlusion" : "closest hit"}; rays redone by the exact kernel: ${res.deferred}\n`);
} else if (cmd === "views") {
  if (rest.length < 7) usage();
  const renderer = require("./renderer.js");
  const [vf, camFile, vw, vh, vrpp, vpasses, vout] = [rest[0], rest[1], +rest[2], +rest[3], +rest[4], +rest[5], rest[6]];
  const raw = fs.readFileSync(camFile);
  const eyes = rest.includes("--eyes"), per = eyes ? 12 : 48;
  if (raw.length % per) { process.stderr.write(`${camFile}: ${raw.length} bytes is not a whole number of ${per}-byte ${eyes ? "eyes" : "cameras"}\n`); process.exit(2); }
  const cameras = new Float32Array(raw.length / 4);
  Buffer.from(cameras.buffer).set(raw);   // (a file's bytes need not sit 4-byte aligned in node's pool)
  const num = (flag, dflt) => { const i = rest.indexOf(flag); if (i < 0) return dflt; const v = Number(rest[i + 1]); if (!Number.isInteger(v) || v < 0) usage(); return v; };
  const pi = rest.indexOf("--ppm");
  if (pi >= 0 && !rest[pi + 1]) usage();
  const bopt = { view: viewOptions(rest), eyes: eyes, bounces: num("--bounces", 5), seedBase: num("--seed-base", 0), countDeferred: true };
  let j, guidesPrefix = null, aoPrefix = null;
  if ((j = rest.indexOf("--guides")) >= 0) {   // the frames' first-hit guides, from the first pass (mirt_render_view_guided_batch)
    if (!rest[j + 1]) usage();
    guidesPrefix = rest[j + 1];
    bopt.guides = true;
  }
  if ((j = rest.indexOf("--ao")) >= 0) {   // the frames' ambient occlusion (mirt_view_ao_batch), before the first pass
    if (!rest[j + 1]) usage();
    aoPrefix = rest[j + 1];
    bopt.ao = {};
    if ((j = rest.indexOf("--ao-samples")) >= 0) bopt.ao.samples = +rest[j + 1];
    if ((j = rest.indexOf("--ao-radius")) >= 0) bopt.ao.radius = +rest[j + 1];
    if ((j = rest.indexOf("--ao-bias")) >= 0) bopt.ao.bias = +rest[j + 1];
  }
  let res;
  try {
    res = renderer.renderViewBatchFile(vf, cameras, vw, vh, vrpp, vpasses, bopt);
  } catch (e) { process.stderr.write(e.message + "\n"); process.exit(2); }
  const bdump = (name, a) => fs.writeFileSync(name, Buffer.from(a.buffer, a.byteOffset, a.byteLength));
  bdump(vout, res.radiance);
  if (res.guides) { bdump(`${guidesPrefix}.normal_hits.f32`, res.guides.normalHits); bdump(`${guidesPrefix}.albedo_depth.f32`, res.guides.albedoDepth); }
  if (res.ao) bdump(`${aoPrefix}.ao.u32`, res.ao.pairs);
  if (pi >= 0) for (let f = 0; f < res.frames; f++) writeFrame(`${rest[pi + 1]}.${f}.ppm`, res.pixel.subarray(f * vw * vh * 4, (f + 1) * vw * vh * 4), vw, vh);
  process.stderr.write(`rendered ${res.frames} ${vw}x${vh} frames of ${vf}, rpp ${vrpp}, ${vpasses} pass(es), ${rest[rest.indexOf("--view") + 1]} cameras: ${res.ms.toFixed(2)} ms on ${res.device}; rays redone by the exact kernel: ${res.deferred}\n`);
  if (res.guidedViews !== undefined) process.stderr.write(`batch calls that wrote their guides: ${res.guidedViews}\n`);
  if (res.ao) process.stderr.write(`ambient occlusion of ${res.frames} frames; pixels redone by the exact kernel: ${res.ao.deferred}\n`);
} else if (cmd === "devices") {
  const { webcl } = require("./webcl.js");
  for (const p of webcl.getPlatforms()) {
    console.log(p.getInfo(webcl.PLATFORM_NAME), "|", p.getInfo(webcl.PLATFORM_VENDOR), "|", p.getInfo(webcl.PLATFORM_VERSION));
    for (const d of p.getDevices(webcl.DEVICE_TYPE_ALL)) console.log("  device:", d.getInfo(webcl.DEVICE_NAME));
  }
} else usage();
