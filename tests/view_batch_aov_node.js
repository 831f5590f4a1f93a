#!/usr/bin/env node
// tests/view_batch_aov_node.js <scene.xml> <cameras.f32> <W> <H> <raysPerPixel> <out-prefix> <model> -- run by tests/test_view_batch_aov_hosts.py:
// queue.viewGuidesBatch (the N-API viewGuidesBatch entry, mirt_view_guides_batch) through renderer.viewGuidesBatchFile, three times -- both
// outputs, normalHits alone, albedoDepth alone -- each result written raw as <out-prefix>.<call>.<output>.f32.  Exits 1 where a call returns an
// output it was not asked for.
const fs = require("fs");
const path = require("path");
const renderer = require(path.join(__dirname, "..", "2015-raytracing_amd", "host", "renderer.js"));
const [file, camFile, w, h, rpp, prefix, model] = process.argv.slice(2);
const raw = fs.readFileSync(camFile);
const cameras = new Float32Array(raw.length / 4);
Buffer.from(cameras.buffer).set(raw);
const calls = { both: {}, nh_alone: { albedoDepth: false }, ad_alone: { normalHits: false } };
for (const [name, opt] of Object.entries(calls)) {
  const res = renderer.viewGuidesBatchFile(file, cameras, +w, +h, +rpp, Object.assign({ view: { model: model } }, opt));
  if ((opt.normalHits === false) !== (res.normalHits === null) || (opt.albedoDepth === false) !== (res.albedoDepth === null)) { process.stderr.write(`${name}: an output that was not asked for\n`); process.exit(1); }
  for (const [out, a] of [["normal_hits", res.normalHits], ["albedo_depth", res.albedoDepth]])
    if (a) fs.writeFileSync(`${prefix}.${name}.${out}.f32`, Buffer.from(a.buffer, a.byteOffset, a.byteLength));
}
