#!/usr/bin/env node
// tests/view_guides_node.js <scene.xml> <W> <H> <raysPerPixel> <out-prefix> <model> <fov> <look x,y,z> -- run by tests/test_view_guides_hosts.py:
// queue.viewGuides (the N-API viewGuides entry, mirt_view_guides) through renderer.viewGuidesFile, three times -- both outputs, normalHits alone,
// albedoDepth alone -- each result written raw as <out-prefix>.<call>.<output>.f32.  Exits 1 where a call returns an output it was not asked for.
const fs = require("fs");
const path = require("path");
const renderer = require(path.join(__dirname, "..", "2015-raytracing_amd", "host", "renderer.js"));
const [file, w, h, rpp, prefix, model, fov, look] = process.argv.slice(2);
const view = { model: model, fov: +fov, look: look.split(",").map(Number) };
const calls = { both: {}, nh_alone: { albedoDepth: false }, ad_alone: { normalHits: false } };
for (const [name, opt] of Object.entries(calls)) {
  const res = renderer.viewGuidesFile(file, +w, +h, +rpp, Object.assign({ view: view }, opt));
  if ((opt.normalHits === false) !== (res.normalHits === null) || (opt.albedoDepth === false) !== (res.albedoDepth === null)) { process.stderr.write(`${name}: an output that was not asked for\n`); process.exit(1); }
  for (const [out, a] of [["normal_hits", res.normalHits], ["albedo_depth", res.albedoDepth]])
    if (a) fs.writeFileSync(`${prefix}.${name}.${out}.f32`, Buffer.from(a.buffer, a.byteOffset, a.byteLength));
}
